// Host test of the encode plan (flo_amd/csrc/encode_plan.cpp): the kernel choices of a lossy batch encode and of
// finish_files pinned as tables, and the invariants checked over the whole input space. Built with g++ by
// tests/test_encode_plan_cpu.py; prints "ok" and exits 0 when everything holds.
#include <cstdio>
#include <string>

#include "../../flo_amd/csrc/encode_plan.hpp"

using namespace flo;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            fprintf(stderr, "FAIL %s: ", #cond);           \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
        }                                                  \
    } while (0)

static const char *name(Chain2qKernel k) {
    static const char *n[] = {"None", "InCoeffs", "Debug", "Dirty44k", "Generic"};
    return n[(int)k];
}
static const char *name(ChainKernel k) {
    static const char *n[] = {"None", "Mono", "MonoExact", "Stereo", "StereoExact"};
    return n[(int)k];
}
static const char *name(FrameKernel k) {
    static const char *n[] = {"None", "Mono1", "Mono2", "Mono2Exact", "Stereo1", "Stereo2", "Stereo2Exact", "Pair1", "Pair2",
                              "Pair2FromCoef", "Multi1", "Multi2", "Multi2Exact"};
    return n[(int)k];
}
static const char *name(CompactKernel k) {
    static const char *n[] = {"None", "Fused", "Offsets1024", "Offsets256"};
    return n[(int)k];
}

static std::string describe(const LossyPlan &p) {
    std::string s;
    switch (p.form) {
    case LossyForm::Chain2q:
        s = std::string("chain2q:") + name(p.chain2q);
        if (p.crc_ready) s += " ready";
        if (p.tail_crc) s += " tail";
        break;
    case LossyForm::Chain: s = std::string("chain:") + name(p.chain); break;
    case LossyForm::Frames:
        s = std::string("frames:") + name(p.pass1) + "," + name(p.pass2);
        if (p.coef_handover) s += " coef";
        if (p.scan()) s += " scan";
        s += std::string(" ") + name(p.compact);
        break;
    }
    return s;
}
static std::string describe(const FinishPlan &f) {
    return std::string(f.fused ? "fused" : f.crc_slices ? "slices" : "noslices") + " " + std::to_string(f.threads) + " " +
           std::to_string(f.parts);
}

struct Row {
    int which, force_path;
    unsigned ch;
    size_t n_clips;
    uint64_t total_frames;
    bool exact, in_coeffs, debug;
    uint32_t dirty;
    bool tail;
    const char *want;
};

constexpr uint32_t D44 = kDirty44k, DANY = 0x7FFFu;
// 256 MiB of 8 KB frames: the largest batch whose frame-parallel stereo form hands coefficients from pass 1 to pass 2
constexpr uint64_t HO = ((uint64_t)256 << 20) / 8192;

static const Row kRows[] = {
    // auto (which 0, nothing forced): n_clips * ch >= 512 takes the chain forms
    {0, 0, 1, 1, 200, 0, 0, 0, D44, 1, "frames:Mono1,Mono2 scan Fused"},
    {0, 0, 1, 16, 3200, 0, 0, 0, D44, 1, "frames:Mono1,Mono2 scan Fused"},
    {0, 0, 1, 17, 3400, 0, 0, 0, D44, 1, "frames:Mono1,Mono2 scan Offsets1024"},
    {0, 0, 1, 511, 102200, 0, 0, 0, D44, 1, "frames:Mono1,Mono2 scan Offsets256"},
    {0, 0, 1, 512, 102400, 0, 0, 0, D44, 1, "chain:Mono"},
    {0, 0, 1, 10000, 2000000, 0, 0, 0, D44, 1, "chain:Mono"},
    {0, 0, 2, 1, 7752, 0, 0, 0, D44, 1, "frames:Pair1,Pair2FromCoef coef Fused"},
    {0, 0, 2, 16, 3200, 0, 0, 0, D44, 1, "frames:Pair1,Pair2FromCoef coef Fused"},
    {0, 0, 2, 17, 3400, 0, 0, 0, D44, 1, "frames:Pair1,Pair2FromCoef coef Offsets1024"},
    {0, 0, 2, 63, 12600, 0, 0, 0, D44, 1, "frames:Pair1,Pair2FromCoef coef Offsets1024"},
    {0, 0, 2, 64, 12800, 0, 0, 0, D44, 1, "frames:Pair1,Pair2FromCoef coef Offsets256"},
    {0, 0, 2, 255, 51000, 0, 0, 0, D44, 1, "frames:Pair1,Pair2 scan Offsets256"},
    {0, 0, 2, 256, 51200, 0, 0, 0, D44, 1, "chain2q:Dirty44k ready tail"},
    {0, 0, 2, 10000, 2000000, 0, 0, 0, D44, 1, "chain2q:Dirty44k ready tail"},
    {0, 0, 2, 10000, 2000000, 0, 0, 0, D44, 0, "chain2q:Dirty44k ready"},
    {0, 0, 2, 10000, 2000000, 0, 0, 0, DANY, 1, "chain2q:Generic ready tail"},
    {0, 0, 3, 4, 800, 0, 0, 0, D44, 1, "frames:Multi1,Multi2 scan Fused"},
    {0, 0, 3, 170, 34000, 0, 0, 0, D44, 1, "frames:Multi1,Multi2 scan Offsets256"},
    {0, 0, 3, 171, 34200, 0, 0, 0, D44, 1, "frames:Multi1,Multi2 scan Offsets256"},
    {0, 0, 8, 64, 12800, 0, 0, 0, D44, 1, "frames:Multi1,Multi2 scan Offsets256"},
    {0, 0, 8, 10000, 2000000, 0, 0, 0, D44, 1, "frames:Multi1,Multi2 scan Offsets256"},
    // the coefficient hand-over limit
    {0, 0, 2, 1, HO, 0, 0, 0, D44, 1, "frames:Pair1,Pair2FromCoef coef Fused"},
    {0, 0, 2, 1, HO + 1, 0, 0, 0, D44, 1, "frames:Pair1,Pair2 scan Fused"},
    {2, 0, 2, 63, HO + 1, 0, 0, 0, D44, 1, "frames:Pair1,Pair2 scan Offsets1024"},
    // forced forms
    {1, 0, 1, 1, 200, 0, 0, 0, D44, 1, "chain:Mono"},
    {1, 0, 2, 1, 200, 0, 0, 0, D44, 1, "chain:Stereo"},
    {1, 0, 2, 10000, 2000000, 1, 0, 0, D44, 1, "chain:StereoExact"},
    {2, 0, 2, 10000, 2000000, 0, 0, 0, D44, 1, "frames:Pair1,Pair2 scan Offsets256"},
    {2, 0, 1, 10000, 2000000, 0, 0, 0, D44, 1, "frames:Mono1,Mono2 scan Offsets256"},
    {3, 0, 2, 16, 3200, 0, 0, 0, D44, 1, "chain2q:Dirty44k"},
    {4, 0, 2, 63, 12600, 0, 0, 0, D44, 1, "chain2q:Dirty44k"},
    {5, 0, 2, 63, 12600, 0, 0, 0, D44, 1, "chain2q:Dirty44k"},
    {5, 0, 2, 64, 12800, 0, 0, 0, D44, 1, "chain2q:Dirty44k ready tail"},
    {5, 0, 2, 64, 12800, 0, 0, 0, D44, 0, "chain2q:Dirty44k ready"},
    {5, 0, 2, 1, 200, 0, 0, 0, DANY, 1, "chain2q:Generic"},
    {5, 0, 1, 64, 12800, 0, 0, 0, D44, 1, "chain:Mono"},
    {3, 0, 1, 1, 200, 0, 0, 0, D44, 1, "chain:Mono"},
    {5, 0, 2, 64, 12800, 1, 0, 0, D44, 1, "chain:StereoExact"},
    {5, 0, 3, 4, 800, 0, 0, 0, D44, 1, "frames:Multi1,Multi2 scan Fused"},
    {1, 0, 8, 4, 800, 0, 0, 0, D44, 1, "frames:Multi1,Multi2 scan Fused"},
    {2, 0, 2, 1, 200, 1, 0, 0, D44, 1, "frames:Stereo1,Stereo2Exact coef scan Fused"},
    // the context's forced form stands in for which = 0; an explicit which wins over it
    {0, 5, 2, 1, 200, 0, 0, 0, D44, 1, "chain2q:Dirty44k"},
    {0, 3, 2, 10000, 2000000, 0, 0, 0, D44, 0, "chain2q:Dirty44k ready"},
    {0, 1, 2, 10000, 2000000, 0, 0, 0, D44, 1, "chain:Stereo"},
    {0, 2, 2, 10000, 2000000, 0, 0, 0, D44, 1, "frames:Pair1,Pair2 scan Offsets256"},
    {0, 1, 1, 1, 200, 0, 0, 0, D44, 1, "chain:Mono"},
    {2, 5, 2, 1, 200, 0, 0, 0, D44, 1, "frames:Pair1,Pair2FromCoef coef Fused"},
    {1, 2, 2, 1, 200, 0, 0, 0, D44, 1, "chain:Stereo"},
    // the analysis entry points (debug buffers): which = 0 is the forced form, else form 1
    {0, 0, 1, 1, 200, 0, 0, 1, D44, 1, "chain:Mono"},
    {0, 0, 2, 1, 200, 0, 0, 1, D44, 1, "chain:Stereo"},
    {0, 0, 2, 1, 200, 1, 1, 1, D44, 1, "chain:StereoExact"},
    {0, 0, 3, 1, 200, 0, 0, 1, D44, 1, "frames:Multi1,Multi2 scan Fused"},
    {0, 5, 2, 1, 200, 0, 0, 1, D44, 1, "chain2q:Debug"},
    {0, 5, 2, 1, 200, 0, 1, 1, D44, 1, "chain2q:InCoeffs"},
    {0, 5, 2, 1, 200, 1, 1, 1, D44, 1, "chain:StereoExact"},
    {0, 2, 2, 1, 200, 0, 0, 1, D44, 1, "frames:Pair1,Pair2FromCoef coef Fused"},
    {0, 2, 2, 1, 200, 0, 1, 1, D44, 1, "frames:Stereo1,Stereo2 coef scan Fused"},
    {0, 2, 2, 1, 200, 1, 1, 1, D44, 1, "frames:Stereo1,Stereo2Exact coef scan Fused"},
    {0, 2, 1, 1, 200, 1, 1, 1, D44, 1, "frames:Mono1,Mono2Exact scan Fused"},
    {0, 2, 3, 1, 200, 1, 1, 1, D44, 1, "frames:Multi1,Multi2Exact scan Fused"},
    {0, 1, 1, 1, 200, 0, 1, 1, D44, 1, "chain:Mono"},
};

static LossyPlanInput input(const Row &r) {
    LossyPlanInput in;
    in.which = r.which;
    in.force_path = r.force_path;
    in.ch = r.ch;
    in.n_clips = r.n_clips;
    in.total_frames = r.total_frames;
    in.exact = r.exact;
    in.in_coeffs = r.in_coeffs;
    in.debug = r.debug;
    in.dirty = r.dirty;
    in.tail_crc = r.tail;
    return in;
}

struct FinishRow {
    size_t n_clips;
    unsigned max_frames;
    bool crc_ready;
    const char *want;
};
static const FinishRow kFinishRows[] = {
    {1, 7752, 0, "fused 1024 512"},     {1, 0, 0, "slices 1024 512"},      {16, 100, 0, "fused 1024 128"},
    {17, 100, 0, "fused 1024 121"},     {63, 100, 0, "fused 1024 33"},     {63, 100, 1, "fused 1024 33"},
    {63, 0, 1, "slices 1024 33"},       {64, 100, 0, "slices 256 32"},     {64, 100, 1, "noslices 256 32"},
    {255, 100, 1, "noslices 256 9"},    {256, 100, 0, "slices 256 8"},     {1023, 100, 0, "slices 256 3"},
    {1024, 100, 1, "noslices 256 1"},   {10000, 100, 0, "slices 256 1"},   {10000, 0, 1, "noslices 256 1"},
};

int main() {
    for (const Row &r : kRows) {
        const std::string got = describe(plan_lossy(input(r)));
        CHECK(got == r.want, "which %d force %d ch %u n %zu frames %llu exact %d in_coeffs %d debug %d dirty %x tail %d: got '%s', want '%s'",
              r.which, r.force_path, r.ch, r.n_clips, (unsigned long long)r.total_frames, r.exact, r.in_coeffs, r.debug, r.dirty,
              r.tail, got.c_str(), r.want);
    }
    for (const FinishRow &r : kFinishRows) {
        const std::string got = describe(plan_finish(r.n_clips, r.max_frames, r.crc_ready));
        CHECK(got == r.want, "n %zu max_frames %u crc_ready %d: got '%s', want '%s'", r.n_clips, r.max_frames, r.crc_ready, got.c_str(),
              r.want);
    }
    // the FLO_CHAIN2X_CLIPS override reaches the lock-step form only
    {
        LossyPlanInput in = input(kRows[13]);
        in.chain2q_clips = 3;
        CHECK(plan_lossy(in).chain2q_clips == 3, "chain2q clips override");
        in.which = 1;
        CHECK(plan_lossy(in).chain2q_clips == 0, "chain2q clips override outside the lock-step form");
    }

    // invariants over the input space
    const unsigned chs[] = {1, 2, 3, 8};
    const size_t ns[] = {0, 1, 16, 17, 63, 64, 170, 171, 255, 256, 511, 512, 1023, 1024, 10000};
    const uint64_t frames_per_clip[] = {1, 200, 7752};
    long cases = 0;
    for (unsigned ch : chs)
        for (size_t n : ns)
            for (uint64_t fpc : frames_per_clip)
                for (int which = 0; which <= 5; which++)
                    for (int fp = 0; fp <= 5; fp++)
                        for (int bits = 0; bits < 32; bits++) {
                            LossyPlanInput in;
                            in.which = which;
                            in.force_path = fp;
                            in.ch = ch;
                            in.n_clips = n;
                            in.total_frames = n * fpc;
                            in.exact = bits & 1;
                            in.in_coeffs = bits & 2;
                            in.debug = bits & 4;
                            in.tail_crc = bits & 8;
                            in.dirty = bits & 16 ? kDirty44k : DANY;
                            const LossyPlan p = plan_lossy(in);
                            const std::string d = describe(p);
                            cases++;
                            const bool frames = p.form == LossyForm::Frames;
                            // exactly the stages of the chosen form are named
                            CHECK((p.chain2q != Chain2qKernel::None) == (p.form == LossyForm::Chain2q), "%s", d.c_str());
                            CHECK((p.chain != ChainKernel::None) == (p.form == LossyForm::Chain), "%s", d.c_str());
                            CHECK((p.pass1 != FrameKernel::None) == frames && (p.pass2 != FrameKernel::None) == frames, "%s", d.c_str());
                            CHECK((p.compact != CompactKernel::None) == frames, "%s", d.c_str());
                            // pass 2 scans itself exactly when it is lossy_frame2x_kernel<2, true>, which needs the hand-over buffer
                            if (frames) CHECK(p.scan() != (p.pass2 == FrameKernel::Pair2FromCoef), "%s", d.c_str());
                            CHECK(!(p.pass2 == FrameKernel::Pair2FromCoef) || p.coef_handover, "%s", d.c_str());
                            CHECK(!p.coef_handover || (frames && ch == 2), "%s", d.c_str());
                            // exact never names the lock-step kernels
                            if (in.exact) {
                                CHECK(p.chain2q == Chain2qKernel::None, "exact: %s", d.c_str());
                                CHECK(p.pass1 != FrameKernel::Pair1 && p.pass2 != FrameKernel::Pair2 && p.pass2 != FrameKernel::Pair2FromCoef,
                                      "exact: %s", d.c_str());
                                CHECK(p.chain != ChainKernel::Mono && p.chain != ChainKernel::Stereo, "exact: %s", d.c_str());
                                CHECK(!frames || p.pass2 == FrameKernel::Mono2Exact || p.pass2 == FrameKernel::Stereo2Exact ||
                                          p.pass2 == FrameKernel::Multi2Exact, "exact: %s", d.c_str());
                            }
                            CHECK(!in.in_coeffs || (p.pass1 != FrameKernel::Pair1 && p.pass2 != FrameKernel::Pair2FromCoef), "in_coeffs: %s",
                                  d.c_str());
                            // the lock-step forms take two channels; more than two always run frame-parallel
                            CHECK(p.form != LossyForm::Chain2q || ch == 2, "%s", d.c_str());
                            CHECK(ch <= 2 || frames, "%s", d.c_str());
                            // the encode's tail computes CRCs only where finish_files reads the ready words
                            CHECK(!p.tail_crc || p.crc_ready, "%s", d.c_str());
                            CHECK(p.crc_ready == (p.form == LossyForm::Chain2q && n >= kFewClips), "%s", d.c_str());
                            CHECK(p.tail_crc == (p.crc_ready && in.tail_crc), "%s", d.c_str());
                            for (unsigned mf : {0u, 1u, (unsigned)fpc}) {
                                const FinishPlan f = plan_finish(n, mf, p.crc_ready);
                                // crc_slices is skipped only when the encode's tail left the CRCs (or crc_and_toc computes them)
                                CHECK(f.crc_slices || f.fused || p.crc_ready, "n %zu: %s", n, d.c_str());
                                CHECK(!(f.crc_slices && f.fused), "n %zu", n);
                                CHECK(f.parts >= 1 && f.parts <= (n < kFewClips ? 512u : 128u) && f.parts == finish_parts(n), "n %zu", n);
                                CHECK(f.threads == (n < kFewClips ? 1024u : 256u), "n %zu", n);
                            }
                        }
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("ok: %zu rows, %zu finish rows, %ld invariant cases\n", sizeof kRows / sizeof kRows[0], sizeof kFinishRows / sizeof kFinishRows[0],
           cases);
    return 0;
}
