// fftconv_plan_test.cpp — the host side of the partitioned FFT convolution (flo_amd/csrc/fftconv_plan.cpp with conv_plan.cpp):
// that every refusal names its quantity; Pn, the segment ranges and the block counts at and around one and two blocks and
// lane_blocks blocks; the skip clamp; the deduplicated responses; grouping under several caps and under one too small for the call, with every block in exactly one
// entry of one group, the stored segments those blocks need and no scratch shared; the scratch sizes; the work lists; the
// twiddle table within half an f32 ulp of f64; the descriptors' sizes and the geometry.
// Prints "ok <checks>" and returns 0, or names the first case that fails.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../flo_amd/csrc/fftconv_plan.hpp"

using namespace flo;

static int g_checks = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        g_checks++;                            \
        if (!(cond)) {                         \
            fprintf(stderr, __VA_ARGS__);      \
            fprintf(stderr, "\n");             \
            return false;                      \
        }                                      \
    } while (0)

static const int64_t B = kFcBlock, LB = kFcLaneBlocks;

static flo_conv_job job(uint32_t clip, uint32_t ir, uint64_t frames, uint64_t skip = 0, uint64_t ir_start = 0, uint32_t taps = UINT32_MAX,
                        uint32_t reserved = 0) {
    flo_conv_job j;
    memset(&j, 0, sizeof j);
    j.clip = clip;
    j.ir = ir;
    j.frames = frames;
    j.skip = skip;
    j.ir_start = ir_start;
    j.taps = taps;
    j.reserved = reserved;
    return j;
}

struct Sources {
    std::vector<uint64_t> a, b;
    int ctx = 0;
    ConvSource src, irs;
    Sources(std::vector<uint64_t> clips, std::vector<uint64_t> resp, uint32_t ch = 2, uint32_t ir_ch = 1) : a(std::move(clips)), b(std::move(resp)) {
        src.present = irs.present = true;
        src.ctx = irs.ctx = &ctx;
        src.rate = irs.rate = 48000;
        src.channels = ch;
        irs.channels = ir_ch;
        src.n_clips = a.size();
        src.clip_frames = a.data();
        irs.n_clips = b.size();
        irs.clip_frames = b.data();
    }
};

static bool refused(const ConvSource &src, const ConvSource &irs, const std::vector<flo_conv_job> &jobs, const char *word, bool null_jobs = false) {
    FcPlan P;
    std::string err;
    const bool ok = fftconv_plan(src, irs, jobs.size(), null_jobs ? nullptr : jobs.data(), kFcGroupBytes, P, err);
    CHECK(!ok, "expected a refusal that names %s", word);
    CHECK(err.find(word) != std::string::npos, "the refusal \"%s\" does not name %s", err.c_str(), word);
    return true;
}

static bool check_refusals() {
    Sources S({1000, 0, 10}, {5, 0, 70, 2000000});
    const std::vector<flo_conv_job> good = {job(0, 0, 100), job(0, 3, 10, 0, 0, FLO_CONV_FFT_MAX_TAPS), job(0, 3, 10, 0, 2000000 - FLO_CONV_FFT_MAX_TAPS)};
    FcPlan P;
    std::string err;
    CHECK(fftconv_plan(S.src, S.irs, good.size(), good.data(), kFcGroupBytes, P, err), "a good list is refused: %s", err.c_str());
    CHECK(P.jobs[1].taps == FLO_CONV_FFT_MAX_TAPS && P.jobs[2].taps == FLO_CONV_FFT_MAX_TAPS && P.jobs[1].parts == FLO_CONV_FFT_MAX_TAPS / B, "the limit itself");
    ConvSource bad = S.src;
    bad.present = false;
    if (!refused(bad, S.irs, good, "src is NULL")) return false;
    if (!refused(S.src, bad, good, "irs is NULL")) return false;
    int other = 0;
    bad = S.irs;
    bad.ctx = &other;
    if (!refused(S.src, bad, good, "context")) return false;
    bad = S.irs;
    bad.rate = 44100;
    if (!refused(S.src, bad, good, "sample_rate")) return false;
    bad = S.src;
    bad.channels = 9;
    if (!refused(bad, S.irs, good, "channels 9")) return false;
    bad = S.irs;
    bad.channels = 3;
    if (!refused(S.src, bad, good, "ir_channels 3")) return false;
    if (!refused(S.src, S.irs, good, "jobs is NULL", true)) return false;
    if (!refused(S.src, S.irs, {job(3, 0, 4)}, "clip 3 of job 0")) return false;
    if (!refused(S.src, S.irs, {job(0, 0, 4), job(0, 4, 4)}, "ir 4 of job 1")) return false;
    if (!refused(S.src, S.irs, {job(0, 0, 4, 0, 0, 1, 1)}, "reserved of job 0")) return false;
    if (!refused(S.src, S.irs, {job(0, 3, 4)}, "FLO_CONV_FFT_MAX_TAPS 1048576")) return false;
    if (!refused(S.src, S.irs, {job(0, 3, 4, 0, 0, FLO_CONV_FFT_MAX_TAPS + 1)}, "taps of job 0: 1048577 taps")) return false;
    if (!refused(S.src, S.irs, {job(0, 0, ~0ull - 3, 4)}, "frames + skip of job 0")) return false;
    if (!refused(S.src, S.irs, {job(0, 0, SIZE_MAX / 16 + 1)}, "frames ")) return false;
    if (!refused(S.src, S.irs, {job(0, 0, 1ull << 45)}, "too many tiles")) return false;
    CHECK(fftconv_plan(S.src, S.irs, 0, nullptr, kFcGroupBytes, P, err) && P.groups.empty() && P.entries.empty() && P.h_elems == 0, "no jobs");
    return true;
}

// every block of every job lies in exactly one entry; entries start at tile boundaries, hold the segments their blocks need
// and nothing of another entry's scratch; groups partition the entries in order
static bool check_cover(const FcPlan &P, const std::vector<flo_conv_job> &jobs, uint64_t cap, const char *what) {
    const uint64_t seg = fftconv_segment_elems(P.channels);
    std::vector<uint64_t> next(jobs.size(), 0);
    size_t at = 0;
    uint64_t most = 0;
    for (const FcGroup &G : P.groups) {
        CHECK(G.first == at && G.count > 0, "%s: the groups partition the entries", what);
        at += G.count;
        uint64_t off = 0;
        for (size_t i = G.first; i < G.first + G.count; i++) {
            const FcEntry &E = P.entries[i];
            const FcJob &J = P.jobs[E.job];
            CHECK(E.b0 == next[E.job] && E.b1 > E.b0 && E.b1 <= J.blocks && E.b0 % LB == 0, "%s: entry %zu follows its job's last", what, i);
            CHECK(E.b1 == J.blocks || E.b1 % LB == 0, "%s: entry %zu is cut at a tile boundary", what, i);
            CHECK(i == G.first || P.entries[i - 1].job <= E.job, "%s: jobs in order", what);
            next[E.job] = E.b1;
            CHECK(E.x_off == off && E.s1 >= E.s0, "%s: entry %zu's scratch follows the one before", what, i);
            off += (uint64_t)(E.s1 - E.s0) * seg;
            // the segments its blocks need: q in [b0 - Pn + 1, b1) that are not zero
            const int64_t lo = std::max<int64_t>(J.q_lo, (int64_t)E.b0 - (int64_t)J.parts + 1), hi = std::min<int64_t>(J.q_hi, (int64_t)E.b1);
            if (hi > lo) CHECK(E.s0 == lo && E.s1 == hi, "%s: entry %zu stores [%lld, %lld), needs [%lld, %lld)", what, i, (long long)E.s0, (long long)E.s1, (long long)lo, (long long)hi);
            else CHECK(E.s0 == E.s1, "%s: entry %zu needs no segment", what, i);
        }
        CHECK(G.x_elems == off, "%s: a group's scratch is its entries'", what);
        // the cap holds unless the group is one entry of one tile
        const FcEntry &E0 = P.entries[G.first];
        CHECK(off * 8 <= cap || (G.count == 1 && E0.b1 - E0.b0 <= (uint64_t)LB), "%s: a group of %llu bytes under a cap of %llu", what,
              (unsigned long long)(off * 8), (unsigned long long)cap);
        most = std::max(most, off);
        std::vector<uint32_t> ps, pm;
        CHECK(fftconv_group_tiles(P, G, ps, pm) && ps.size() == G.count + 1 && pm.size() == G.count + 1, "%s: the lists", what);
        for (size_t i = 0; i < G.count; i++) {
            const FcEntry &E = P.entries[G.first + i];
            const uint64_t items = (uint64_t)(E.s1 - E.s0) * P.channels;
            CHECK(ps[i + 1] - ps[i] == (items + kFcTogether - 1) / kFcTogether, "%s: transform tiles", what);
            CHECK(pm[i + 1] - pm[i] == (E.b1 - E.b0 + LB - 1) / LB, "%s: block tiles", what);
        }
    }
    CHECK(at == P.entries.size() && P.x_elems == most, "%s: every entry is in a group; x_elems is the largest", what);
    for (size_t k = 0; k < jobs.size(); k++) CHECK(next[k] == P.jobs[k].blocks, "%s: job %zu is covered to its end", what, k);
    return true;
}

static bool check_jobs() {
    Sources S({(uint64_t)(3 * LB * B + 5), 0, 1, (uint64_t)(2 * B)}, {(uint64_t)((LB + 1) * B + 1), 0, 7});
    FcPlan P;
    std::string err;
    struct Row {
        flo_conv_job g;
        uint32_t K, Pn;
        uint64_t skip, blocks;
        int64_t q_lo, q_hi;
    };
    const int64_t N0 = 3 * LB * B + 5;
    const std::vector<Row> rows = {
        {job(2, 2, 1, 0, 0, 1), 1, 1, 0, 1, 0, 1},                                  // N = K = T = 1
        {job(3, 0, B, 0, 0, (uint32_t)B), (uint32_t)B, 1, 0, 1, 0, 1},              // one block, one partition
        {job(3, 0, B + 1, 0, 0, (uint32_t)B), (uint32_t)B, 1, 0, 2, 0, 2},
        {job(3, 0, 2 * B, 0, 0, (uint32_t)(B + 1)), (uint32_t)(B + 1), 2, 0, 2, 0, 2},   // q = -1 holds frames [-2B, 0): zero
        {job(3, 0, 2 * B + 1, 0, 0, (uint32_t)(2 * B)), (uint32_t)(2 * B), 2, 0, 3, 0, 3},
        {job(3, 0, 5 * B, 0, 0, (uint32_t)(2 * B)), (uint32_t)(2 * B), 2, 0, 5, 0, 3},   // N = 2B: q = 3 starts at frame 2B
        {job(3, 0, 5 * B, 1, 0, (uint32_t)(2 * B)), (uint32_t)(2 * B), 2, 1, 5, -1, 3},  // skip 1: q = -1 ends at frame 1
        {job(3, 0, 5 * B, B, 0, (uint32_t)(2 * B)), (uint32_t)(2 * B), 2, (uint64_t)B, 5, -1, 2},
        {job(3, 0, 5 * B, B + 1, 0, (uint32_t)(3 * B)), (uint32_t)(3 * B), 3, (uint64_t)(B + 1), 5, -2, 2},
        {job(3, 0, 5 * B, B + 1, 0, (uint32_t)(B)), (uint32_t)B, 1, (uint64_t)(B + 1), 5, 0, 2},   // Pn = 1: no block uses q < 0
        {job(3, 2, B, 1000000), 7, 1, (uint64_t)(2 * B + 7), 1, 0, 1},                   // the clamp N + K: segment 0 still holds frames of the clip
        {job(3, 2, B, 2 * B + 6), 7, 1, (uint64_t)(2 * B + 6), 1, 0, 1},                 // one short of it
        {job(1, 0, 3 * B), (uint32_t)((LB + 1) * B + 1), (uint32_t)(LB + 2), 0, 3, 0, 0},          // N = 0
        {job(0, 1, 3 * B), 0, 0, 0, 3, 0, 0},                                                      // K = 0
        {job(0, 0, 0), (uint32_t)((LB + 1) * B + 1), (uint32_t)(LB + 2), 0, 0, 0, 0},              // T = 0
        {job(0, 0, LB * B, 0, (uint64_t)((LB + 1) * B + 1)), 0, 0, 0, (uint64_t)LB, 0, 0},         // ir_start at P
        {job(0, 0, LB * B + 1, 0, (uint64_t)((LB + 1) * B)), 1, 1, 0, (uint64_t)(LB + 1), 0, LB + 1},   // one tap left
        {job(0, 0, N0 + 4 * B, 0, 1, (uint32_t)(4 * B - 100)), (uint32_t)(4 * B - 100), 4, 0, (uint64_t)(3 * LB + 5), 0, 3 * LB + 2},
    };
    std::vector<flo_conv_job> jobs;
    for (const Row &r : rows) jobs.push_back(r.g);
    CHECK(fftconv_plan(S.src, S.irs, jobs.size(), jobs.data(), kFcGroupBytes, P, err), "the rows are refused: %s", err.c_str());
    for (size_t k = 0; k < rows.size(); k++) {
        const Row &r = rows[k];
        const FcJob &J = P.jobs[k];
        CHECK(J.taps == r.K && J.parts == r.Pn && J.skip == r.skip && J.blocks == r.blocks, "row %zu: K %u Pn %u skip %llu blocks %llu", k, J.taps, J.parts,
              (unsigned long long)J.skip, (unsigned long long)J.blocks);
        CHECK(J.q_lo == r.q_lo && J.q_hi == r.q_hi, "row %zu: segments [%lld, %lld)", k, (long long)J.q_lo, (long long)J.q_hi);
    }
    // responses: one per distinct (ir, ir_start, K); every K == 0 is one
    CHECK(P.jobs[1].response == P.jobs[2].response && P.jobs[3].response != P.jobs[1].response, "equal responses are shared");
    CHECK(P.jobs[13].response == P.jobs[15].response && P.responses[P.jobs[13].response].parts == 0, "K == 0 is one empty response");
    CHECK(P.jobs[10].response == P.jobs[11].response && P.jobs[0].response != P.jobs[10].response, "taps cut by the end are K, not taps");
    uint64_t h = 0;
    for (const FcResponse &R : P.responses) {
        CHECK(R.h_off == h && R.parts == fftconv_parts(R.taps), "the responses' spectra follow one another");
        h += (uint64_t)R.parts * 1 * B;
    }
    CHECK(h == P.h_elems, "h_elems");
    std::vector<uint32_t> pre;
    CHECK(fftconv_response_tiles(P, pre) && pre.size() == P.responses.size() + 1, "response tiles");
    for (size_t r = 0; r < P.responses.size(); r++) CHECK(pre[r + 1] - pre[r] == (P.responses[r].parts + kFcTogether - 1) / kFcTogether, "response %zu's tiles", r);
    if (!check_cover(P, jobs, kFcGroupBytes, "default cap")) return false;
    CHECK(P.groups.size() == 1 && P.entries.size() == rows.size() - 1, "one group; the job without blocks has no entry");
    // smaller caps: in segments of two channels
    const uint64_t seg_bytes = fftconv_segment_elems(2) * 8;
    for (uint64_t segs : {1ull, 2ull, (unsigned long long)LB, (unsigned long long)LB + 1, (unsigned long long)(2 * LB + 3), 1000ull}) {
        FcPlan Q;
        CHECK(fftconv_plan(S.src, S.irs, jobs.size(), jobs.data(), segs * seg_bytes, Q, err), "cap %llu: %s", (unsigned long long)segs, err.c_str());
        if (!check_cover(Q, jobs, segs * seg_bytes, ("cap of " + std::to_string(segs) + " segments").c_str())) return false;
        for (size_t k = 0; k < jobs.size(); k++)
            CHECK(Q.jobs[k].q_lo == P.jobs[k].q_lo && Q.jobs[k].q_hi == P.jobs[k].q_hi && Q.jobs[k].response == P.jobs[k].response, "the cap changes no job");
        if (segs == (uint64_t)(2 * LB + 3)) {   // the last job has 3 LB + 2 segments: it is cut, and there are several groups
            size_t cuts = 0;
            for (const FcEntry &E : Q.entries) cuts += E.job == rows.size() - 1;
            CHECK(cuts >= 2 && Q.groups.size() >= 3, "the long job is cut (%zu entries, %zu groups)", cuts, Q.groups.size());
        }
    }
    return true;
}

// a cap of one segment on a long clip: the cap is raised so that about kFcMaxGroups groups hold the call
static bool check_many_groups() {
    const uint64_t N = (uint64_t)(100000 * LB * B);
    Sources S({N, N}, {(uint64_t)(3 * B)});
    const std::vector<flo_conv_job> jobs = {job(0, 0, N), job(1, 0, N + 3 * B - 1)};
    FcPlan P;
    std::string err;
    CHECK(fftconv_plan(S.src, S.irs, jobs.size(), jobs.data(), 1, P, err), "a cap of one byte: %s", err.c_str());
    uint64_t all = 0;
    for (const FcJob &J : P.jobs) all += (uint64_t)(J.q_hi - J.q_lo);
    const uint64_t cap = ((all + kFcMaxGroups - 1) / kFcMaxGroups) * fftconv_segment_elems(2) * 8;
    CHECK(all > 100 * kFcMaxGroups * (uint64_t)LB, "the case is long enough");
    CHECK(P.groups.size() <= 2 * kFcMaxGroups && P.groups.size() >= kFcMaxGroups / 2, "%zu groups", P.groups.size());
    if (!check_cover(P, jobs, cap, "raised cap")) return false;
    return true;
}

static bool check_twiddles_and_geometry() {
    std::vector<float> tw;
    fftconv_twiddles(tw);
    CHECK(tw.size() == 2 * (size_t)B, "the table has B entries");
    for (int64_t k = 0; k < B; k++) {
        const long double a = 3.14159265358979323846264338327950288L * (long double)k / (long double)B;
        const long double want[2] = {cosl(a), -sinl(a)};
        for (int i = 0; i < 2; i++) {
            const float got = tw[2 * k + i];
            // half an ulp of the f32 nearest to the exact value (plus the f64 evaluation's own 1e-16)
            const float near = (float)want[i];
            const long double half = (long double)(std::nextafter(std::fabs(near), INFINITY) - std::fabs(near)) / 2;
            CHECK(fabsl((long double)got - want[i]) <= half + 1e-16L, "twiddle %lld.%d is %a", (long long)k, i, got);
        }
    }
    CHECK(tw[0] == 1.0f && tw[1] == 0.0f && tw[2 * (B / 2) + 1] == -1.0f, "the exact points");
    flo_conv_fft_info info;
    for (int ch = 1; ch <= 8; ch++)
        for (int ir = 1; ir <= 8; ir++) {
            const int rc = flo_conv_fft_geometry((uint8_t)ch, (uint8_t)ir, &info);
            if (ir == 1 || ir == ch)
                CHECK(rc == 0 && info.block_frames == kFcBlock && info.lane_blocks == kFcLaneBlocks && info.max_taps == FLO_CONV_FFT_MAX_TAPS &&
                          info.crossover_taps == kFcCrossoverTaps, "geometry of %d, %d", ch, ir);
            else
                CHECK(rc != 0, "geometry of %d, %d is refused", ch, ir);
        }
    CHECK(flo_conv_fft_geometry(0, 1, &info) != 0 && flo_conv_fft_geometry(9, 1, &info) != 0 && flo_conv_fft_geometry(2, 1, nullptr) != 0, "refusals");
    CHECK(sizeof(FcSpecJob) == 64 && sizeof(FcMacJob) == 64 && sizeof(flo_conv_fft_info) == 16, "sizes");
    CHECK(kFcTileFrames == kFcBlock * kFcLaneBlocks && kFcBinsPerLane * kFcThreads == kFcBlock, "tile and bins");
    return true;
}

int main() {
    if (!check_refusals() || !check_jobs() || !check_many_groups() || !check_twiddles_and_geometry()) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
