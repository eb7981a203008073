// conv_plan_test.cpp — the host side of the FIR stage (flo_amd/csrc/conv_plan.cpp, fir_design.cpp and the inline functions of
// conv_plan.hpp that the kernel uses): that every refusal names its quantity, the taps of a job for ir_start below, at and
// beyond the response's end and for taps = UINT32_MAX, the kernel's skip, the tile prefix for lengths at and around a tile,
// the LDS index and its bounds, the geometry, and flo_fir_design's refusals and symmetries.
// Prints "ok <checks>" and returns 0, or names the first case that fails.
// With the argument "design" it reads lines "kind rate f_lo f_hi taps beta" and prints for each the table as hexadecimal f32
// bit patterns on one line (tests/test_convolve_cpu.py compares them with numpy's f64 restatement).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../flo_amd/csrc/clip_tiles.hpp"
#include "../../flo_amd/csrc/conv_plan.hpp"

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
    uint64_t a[3] = {1000, 0, 10}, b[4] = {5, 0, 70, 70000};
    int ctx = 0;
    ConvSource src, irs;
    Sources() {
        src.present = irs.present = true;
        src.ctx = irs.ctx = &ctx;
        src.rate = irs.rate = 48000;
        src.channels = 2;
        irs.channels = 1;
        src.n_clips = 3;
        src.clip_frames = a;
        irs.n_clips = 4;
        irs.clip_frames = b;
    }
};

static bool refused(const ConvSource &src, const ConvSource &irs, const std::vector<flo_conv_job> &jobs, const char *word, bool null_jobs = false) {
    std::vector<uint32_t> K, pre;
    std::string err;
    const bool ok = conv_check(src, irs, jobs.size(), null_jobs ? nullptr : jobs.data(), K, pre, err);
    CHECK(!ok, "expected a refusal that names %s", word);
    CHECK(err.find(word) != std::string::npos, "the refusal \"%s\" does not name %s", err.c_str(), word);
    return true;
}

static bool check_refusals() {
    Sources S;
    std::vector<uint32_t> K, pre;
    std::string err;
    const uint64_t F = kConvTileFrames;
    const std::vector<flo_conv_job> good = {job(0, 0, 100), job(2, 2, 0, 7, 3, 20), job(1, 1, 2 * F + 1, ~0ull - 2 * F - 1), job(0, 2, F, 5, 70), job(0, 2, F + 1, 0, 69),
                                            job(0, 3, F - 1, 0, 70000 - 65536), job(0, 3, 1, 0, 0, 65536)};
    CHECK(conv_check(S.src, S.irs, good.size(), good.data(), K, pre, err), "a good list is refused: %s", err.c_str());
    CHECK(K == (std::vector<uint32_t>{5, 20, 0, 0, 1, 65536, 65536}), "the taps of the good list");
    CHECK(pre == (std::vector<uint32_t>{0, 1, 1, 4, 5, 7, 8, 9}), "the prefix of tiles");
    CHECK(conv_check(S.src, S.irs, 0, nullptr, K, pre, err) && K.empty() && pre == std::vector<uint32_t>{0}, "no jobs: %s", err.c_str());
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
    if (!refused(S.src, bad, good, "sample_rate 44100")) return false;
    if (!refused(S.src, bad, good, "resample")) return false;
    bad = S.irs;
    bad.channels = 3;
    if (!refused(S.src, bad, good, "ir_channels 3")) return false;
    bad.channels = 2;
    CHECK(conv_check(S.src, bad, good.size(), good.data(), K, pre, err), "a response of the source's channels is refused: %s", err.c_str());
    bad = S.src;
    bad.channels = 9;
    if (!refused(bad, S.irs, good, "channels 9")) return false;
    bad.channels = 0;
    if (!refused(bad, S.irs, good, "channels 0")) return false;
    if (!refused(S.src, S.irs, good, "jobs is NULL", true)) return false;
    if (!refused(S.src, S.irs, {job(3, 0, 1)}, "clip 3")) return false;
    if (!refused(S.src, S.irs, {job(0, 0, 1), job(0, 4, 1)}, "ir 4 of job 1")) return false;
    if (!refused(S.src, S.irs, {job(0, 0, 1, 0, 0, 1, 1)}, "reserved")) return false;
    if (!refused(S.src, S.irs, {job(0, 3, 1)}, "FLO_CONV_MAX_TAPS")) return false;
    if (!refused(S.src, S.irs, {job(0, 3, 1, 0, 70000 - 65537)}, "taps of job 0")) return false;
    if (!refused(S.src, S.irs, {job(0, 0, 5, ~0ull - 3)}, "frames + skip")) return false;
    const flo_conv_job edge = job(0, 0, 5, ~0ull - 5);
    CHECK(conv_check(S.src, S.irs, 1, &edge, K, pre, err), "a sum of 2^64 - 1 is refused: %s", err.c_str());
    const uint64_t most = (uint64_t)(SIZE_MAX / 8) / 2;
    if (!refused(S.src, S.irs, {job(0, 0, most + 1)}, "frames ")) return false;
    if (!refused(S.src, S.irs, {job(0, 0, 5), job(0, 0, 0x7FFFFFFFull * F), job(0, 0, 1)}, "tiles")) return false;
    const flo_conv_job full = job(0, 0, 0x7FFFFFFFull * F);
    CHECK(conv_check(S.src, S.irs, 1, &full, K, pre, err) && pre[1] == 0x7FFFFFFFu, "2^31 - 1 tiles: %s", err.c_str());
    return true;
}

static bool check_taps_and_skip() {
    CHECK(conv_taps(UINT32_MAX, 70, 0) == 70 && conv_taps(UINT32_MAX, 70, 69) == 1 && conv_taps(UINT32_MAX, 70, 70) == 0, "taps to the end");
    CHECK(conv_taps(UINT32_MAX, 70, 71) == 0 && conv_taps(5, 70, ~0ull) == 0 && conv_taps(UINT32_MAX, 0, 0) == 0, "ir_start beyond the end");
    CHECK(conv_taps(5, 70, 3) == 5 && conv_taps(5, 70, 65) == 5 && conv_taps(5, 70, 66) == 4 && conv_taps(0, 70, 3) == 0, "taps cut by the end");
    CHECK(conv_taps(UINT32_MAX, (1ull << 40), 1) == UINT32_MAX, "a response longer than 2^32");
    CHECK(conv_skip(0, 10, 3) == 0 && conv_skip(12, 10, 3) == 12 && conv_skip(13, 10, 3) == 13 && conv_skip(14, 10, 3) == 13 && conv_skip(~0ull, 0, 0) == 0,
          "the kernel's skip");
    // from skip = N + K on, every tap of every output meets a frame at or past N: t + skip - k >= N + K - (K - 1) > N - 1
    for (uint64_t N : {0ull, 1ull, 10ull})
        for (uint32_t K : {1u, 3u})
            for (uint64_t t : {0ull, 5ull}) CHECK(t + conv_skip(~0ull - 9, N, K) - (K - 1) >= N, "a clamped skip leaves a frame inside the clip");
    return true;
}

static bool check_geometry() {
    CHECK(kConvTileFrames == kConvThreads * kConvLaneOutputs && kConvTapChunk % kConvLaneOutputs == 0, "the geometry's multiples");
    CHECK(kConvStaged == kConvTileFrames + kConvTapChunk - 1 && conv_lds_index(kConvStaged - 1) + 1 == kConvLdsElems, "the staged span");
    CHECK(kConvLdsElems * 8 <= 64 * 1024, "the float2 frames of a chunk fit 64 KB of LDS");
    uint32_t last = 0;
    for (uint32_t s = 1; s < kConvStaged; s++) {   // strictly increasing: no two staged frames share an element
        const uint32_t i = conv_lds_index(s);
        CHECK(i > last && i < kConvLdsElems, "LDS index %u of staged frame %u", i, s);
        last = i;
    }
    // lanes read kConvLaneOutputs frames apart: an odd number of elements, so 32 lanes fall on 32 different banks
    for (uint32_t s0 = 0; s0 < kConvTapChunk + kConvLaneOutputs; s0++) {
        bool bank[32] = {};
        for (uint32_t lane = 0; lane < 32; lane++) {
            const uint32_t i = conv_lds_index(lane * kConvLaneOutputs + s0) % 32;
            CHECK(!bank[i], "two of 32 lanes share bank %u at staged offset %u", i, s0);
            bank[i] = true;
        }
    }
    flo_conv_info g;
    for (int ch = 1; ch <= 8; ch++)
        for (int ir : {1, ch}) {
            CHECK(flo_conv_geometry((uint8_t)ch, (uint8_t)ir, &g) == FLO_OK, "geometry of %d, %d", ch, ir);
            CHECK(g.tile_frames == kConvTileFrames && g.tap_chunk == kConvTapChunk && g.lane_outputs == kConvLaneOutputs, "the geometry in force");
        }
    CHECK(flo_conv_geometry(0, 1, &g) == FLO_ERR_ARG && flo_conv_geometry(9, 1, &g) == FLO_ERR_ARG && flo_conv_geometry(4, 2, &g) == FLO_ERR_ARG &&
              flo_conv_geometry(2, 1, nullptr) == FLO_ERR_ARG,
          "the geometry's refusals");
    std::vector<uint32_t> pre;
    const uint64_t F = kConvTileFrames, T[] = {0, 1, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1};
    CHECK(clip_tiles(T, 8, F, pre) && pre == (std::vector<uint32_t>{0, 0, 1, 2, 3, 5, 7, 9, 12}), "the tile prefix at and around a tile");
    return true;
}

static bool design_refused(uint32_t kind, uint32_t rate, double lo, double hi, uint32_t taps, double beta, const char *word) {
    char err[200] = "";
    float *t = (float *)1;
    const int rc = flo_fir_design(kind, rate, lo, hi, taps, beta, &t, err, sizeof err);
    CHECK(rc == FLO_ERR_ARG && !t, "expected a refusal that names %s", word);
    CHECK(strstr(err, word), "the refusal \"%s\" does not name %s", err, word);
    return true;
}

static bool check_design() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    if (!design_refused(4, 48000, 100, 200, 255, 9, "kind")) return false;
    if (!design_refused(0, 0, 100, 200, 255, 9, "rate")) return false;
    for (uint32_t taps : {0u, 1u, 2u, 4u, 254u, 65536u, 65537u})
        if (!design_refused(0, 48000, 100, 200, taps, 9, "taps")) return false;
    for (double beta : {-0.5, 16.5, nan, inf})
        if (!design_refused(0, 48000, 100, 200, 255, beta, "beta")) return false;
    for (double f : {0.0, -1.0, 24000.0, 30000.0, nan, inf}) {
        if (!design_refused(FLO_FIR_LOWPASS, 48000, 100, f, 255, 9, "f_hi")) return false;
        if (!design_refused(FLO_FIR_HIGHPASS, 48000, f, 100, 255, 9, "f_lo")) return false;
        if (!design_refused(FLO_FIR_BANDPASS, 48000, f, 100, 255, 9, "f_lo")) return false;
        if (!design_refused(FLO_FIR_BANDSTOP, 48000, 100, f, 255, 9, "f_hi")) return false;
    }
    if (!design_refused(FLO_FIR_BANDPASS, 48000, 200, 200, 255, 9, "f_lo must be below f_hi")) return false;
    if (!design_refused(FLO_FIR_BANDSTOP, 48000, 300, 200, 255, 9, "f_lo must be below f_hi")) return false;
    char err[8];
    CHECK(flo_fir_design(0, 48000, 0, 100, 255, 9, nullptr, err, sizeof err) == FLO_ERR_ARG, "a NULL table");
    float *t = nullptr;
    CHECK(flo_fir_design(0, 48000, 0, 100, 4, 9, &t, err, sizeof err) == FLO_ERR_ARG && strlen(err) == 7, "a short error buffer is filled and terminated");
    CHECK(flo_fir_design(0, 48000, 0, 100, 4, 9, &t, nullptr, 0) == FLO_ERR_ARG, "no error buffer");
    // the frequency a kind does not use is ignored; both ends of the allowed ranges are accepted
    for (uint32_t taps : {3u, 255u, 65535u})
        for (double beta : {0.0, 9.0, 16.0}) {
            CHECK(flo_fir_design(FLO_FIR_LOWPASS, 48000, nan, 4000, taps, beta, &t, err, sizeof err) == FLO_OK && t, "a low-pass of %u taps, beta %g: %s", taps, beta, err);
            double sum = 0;
            for (uint32_t k = 0; k < taps; k++) {
                CHECK(std::isfinite(t[k]) && t[k] == t[taps - 1 - k], "tap %u of %u is not finite or not symmetric", k, taps);
                sum += t[k];
            }
            CHECK(std::fabs(sum - 1.0) < 1e-5, "the low-pass sums to %.9g", sum);
            free(t);
        }
    CHECK(flo_fir_design(FLO_FIR_HIGHPASS, 48000, 80, -5, 101, 9, &t, err, sizeof err) == FLO_OK, "a high-pass: %s", err);
    double sum = 0;
    for (uint32_t k = 0; k < 101; k++) sum += t[k];
    CHECK(std::fabs(sum) < 1e-5, "the high-pass sums to %.9g", sum);
    free(t);
    // the kinds are what the definition says of one another: stop = delta - pass, pass = lp(f_hi) - lp(f_lo), high = delta - lp
    std::vector<double> stop, pass, lo, hi, high;
    std::string m;
    CHECK(fir_design(FLO_FIR_BANDSTOP, 44100, 300, 3400, 31, 16.0, stop, m) && fir_design(FLO_FIR_BANDPASS, 44100, 300, 3400, 31, 16.0, pass, m) &&
              fir_design(FLO_FIR_LOWPASS, 44100, 0, 300, 31, 16.0, lo, m) && fir_design(FLO_FIR_LOWPASS, 44100, 0, 3400, 31, 16.0, hi, m) &&
              fir_design(FLO_FIR_HIGHPASS, 44100, 300, 0, 31, 16.0, high, m) && stop.size() == 31,
          "the f64 tables: %s", m.c_str());
    for (size_t k = 0; k < 31; k++) {
        const double delta = k == 15 ? 1.0 : 0.0;
        CHECK(stop[k] == delta - pass[k] && pass[k] == hi[k] - lo[k] && high[k] == delta - lo[k], "tap %zu of the four kinds", k);
    }
    return true;
}

static int design() {
    unsigned kind, rate, taps;
    double lo, hi, beta;
    while (scanf("%u %u %lf %lf %u %lf", &kind, &rate, &lo, &hi, &taps, &beta) == 6) {
        float *t = nullptr;
        char err[200];
        if (flo_fir_design(kind, rate, lo, hi, taps, beta, &t, err, sizeof err) != FLO_OK) {
            fprintf(stderr, "%s\n", err);
            return 1;
        }
        for (unsigned k = 0; k < taps; k++) {
            uint32_t bits;
            memcpy(&bits, &t[k], 4);
            printf("%08x%c", bits, k + 1 == taps ? '\n' : ' ');
        }
        free(t);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "design")) return design();
    if (!check_refusals() || !check_taps_and_skip() || !check_geometry() || !check_design()) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
