// normalize_plan_test.cpp — the host side of loudness normalisation (flo_amd/csrc/normalize_plan.cpp and the inline tile
// geometry of normalize_plan.hpp that the kernel shares): the gain of a clip on a table of cases, the look-ahead defaults,
// that refusals name the quantity, that the tiles of a batch cover every frame exactly once, and that everything a tile
// reads lies inside its staged span and its LDS planes. Prints "ok <checks>" and returns 0, or names the first case that fails.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../flo_amd/csrc/clip_tiles.hpp"
#include "../../flo_amd/csrc/normalize_plan.hpp"

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

static flo_normalize_opts defaults() {
    flo_normalize_opts o;
    std::string err;
    normalize_opts(nullptr, o, err);
    return o;
}

static bool check_defaults() {
    const flo_normalize_opts o = defaults();
    CHECK(o.target_lufs == -14.0 && o.ceiling_dbtp == -1.0 && o.max_gain_db == 30.0 && o.mode == FLO_NORM_GAIN && o.lookahead_frames == 0,
          "the defaults are %g LUFS, %g dBTP, %g dB, mode %u, look-ahead %u", o.target_lufs, o.ceiling_dbtp, o.max_gain_db, o.mode, o.lookahead_frames);
    CHECK(normalize_ceiling(o) == (float)std::pow(10.0, -1.0 / 20.0), "C of -1 dBTP");
    return true;
}

static bool check_gain() {
    const float C = normalize_ceiling(defaults());
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    struct Case {
        const char *name;
        double lufs, sample_peak, target, max_gain;
        float tp;
        uint32_t mode;
        double want_db;      // the clamped gain before the ceiling
        bool lowered;
        uint32_t status;
    };
    const Case cases[] = {
        {"plain", -20.0, -12.0, -14.0, 30.0, 0.25f, FLO_NORM_GAIN, 6.0, false, 0},
        {"down", -8.0, -3.0, -14.0, 30.0, 0.7f, FLO_NORM_GAIN, -6.0, false, 0},
        {"clamp up", -60.0, -50.0, -14.0, 30.0, 0.003f, FLO_NORM_GAIN, 30.0, false, 0},
        {"clamp down", 20.0, 30.0, -14.0, 30.0, 30.0f, FLO_NORM_LIMIT, -30.0, false, 0},
        {"clamp up, narrow", -30.0, -20.0, -14.0, 6.0, 0.1f, FLO_NORM_GAIN, 6.0, false, 0},
        {"max_gain_db 0", -30.0, -20.0, -14.0, 0.0, 0.1f, FLO_NORM_GAIN, 0.0, false, 0},
        {"ceiling cap", -20.0, -2.0, -14.0, 30.0, 0.8f, FLO_NORM_GAIN, 6.0, true, 0},
        {"ceiling cap at gain below 1", -14.0, 0.0, -14.0, 30.0, 1.3f, FLO_NORM_GAIN, 0.0, true, 0},
        {"no cap in LIMIT mode", -20.0, -2.0, -14.0, 30.0, 0.8f, FLO_NORM_LIMIT, 6.0, false, 0},
        {"overflow guard in LIMIT mode", -44.0, 600.0, -14.0, 30.0, 1e30f, FLO_NORM_LIMIT, 30.0, true, 0},
        {"fallback loudness", -23.0, -10.0, -14.0, 30.0, 0.3f, FLO_NORM_GAIN, 9.0, false, 0},
        {"silent", -23.0, -150.0, -14.0, 30.0, 0.0f, FLO_NORM_GAIN, 0.0, false, FLO_NORM_STATUS_SILENT},
        {"silent with a true peak", -70.0, -150.0, -14.0, 30.0, 1e-6f, FLO_NORM_LIMIT, 0.0, false, FLO_NORM_STATUS_SILENT},
        {"NaN loudness", nan, -3.0, -14.0, 30.0, 0.5f, FLO_NORM_GAIN, 0.0, false, FLO_NORM_STATUS_NONFINITE},
        {"-inf loudness", -inf, -3.0, -14.0, 30.0, 0.5f, FLO_NORM_LIMIT, 0.0, false, FLO_NORM_STATUS_NONFINITE},
        {"inf true peak", -20.0, -3.0, -14.0, 30.0, std::numeric_limits<float>::infinity(), FLO_NORM_GAIN, 0.0, false, FLO_NORM_STATUS_NONFINITE},
        {"NaN true peak, silent sample peak", -23.0, -150.0, -14.0, 30.0, std::numeric_limits<float>::quiet_NaN(), FLO_NORM_GAIN, 0.0, false, FLO_NORM_STATUS_NONFINITE},
        {"NaN sample peak", -20.0, nan, -14.0, 30.0, 0.5f, FLO_NORM_GAIN, 0.0, false, FLO_NORM_STATUS_NONFINITE},
    };
    for (const Case &k : cases) {
        flo_normalize_opts o = defaults();
        o.target_lufs = k.target;
        o.max_gain_db = k.max_gain;
        o.mode = k.mode;
        flo_normalize_report r;
        memset(&r, 0xAB, sizeof r);
        normalize_gain(k.lufs, k.sample_peak, k.tp, o, r);
        CHECK(r.status == k.status, "%s: status %u", k.name, r.status);
        CHECK(r.min_gain_q24 == kNormUnity && r.limited_frames == 0, "%s: the kernel's fields start at 2^24 and 0", k.name);
        CHECK(memcmp(&r.input_true_peak, &k.tp, 4) == 0, "%s: input_true_peak", k.name);
        CHECK((std::isnan(k.lufs) && std::isnan(r.input_lufs)) || r.input_lufs == k.lufs, "%s: input_lufs", k.name);
        if (k.status) {
            CHECK(r.gain == 1.0f && r.gain_db == 0.0 && r.ceiling_reduction_db == 0.0, "%s: a copied clip has gain 1", k.name);
            continue;
        }
        const float plain = (float)std::pow(10.0, k.want_db / 20.0);
        const double cap = k.mode == FLO_NORM_GAIN ? (double)C * kNormGainMargin : kNormMaxScaledPeak;
        CHECK(r.gain_db == 20.0 * std::log10((double)r.gain), "%s: gain_db is 20 log10 of gain", k.name);
        CHECK(r.input_true_peak_dbtp == (k.tp > 1e-9f ? 20.0 * std::log10((double)k.tp) : -150.0), "%s: input_true_peak_dbtp", k.name);
        if (!k.lowered) {
            CHECK(r.gain == plain && r.ceiling_reduction_db == 0.0, "%s: gain %.9g, want %.9g", k.name, r.gain, plain);
            CHECK((double)k.tp * r.gain <= cap, "%s: the cap holds without lowering", k.name);
        } else {
            CHECK(r.gain < plain && (double)k.tp * (double)r.gain <= cap, "%s: gain %.9g keeps the true peak at or below %.9g", k.name, r.gain, cap);
            CHECK((double)k.tp * (double)std::nextafterf(r.gain, INFINITY) > cap, "%s: the next gain up would pass the cap", k.name);
            CHECK(r.ceiling_reduction_db > 0.0 && std::fabs(r.ceiling_reduction_db - (k.want_db - r.gain_db)) < 1e-12, "%s: ceiling_reduction_db %g", k.name,
                  r.ceiling_reduction_db);
        }
    }
    return true;
}

static bool check_lookahead() {
    const uint32_t rates[] = {8000, 44100, 48000, 192000, 384000, 1, 333, 334, 1100};
    const uint32_t want[] = {12, 66, 72, 288, 576, 1, 1, 1, 2};
    std::string err;
    for (size_t i = 0; i < sizeof rates / sizeof *rates; i++) {
        uint32_t a = 0;
        CHECK(normalize_lookahead(rates[i], 0, a, err) && a == want[i], "1.5 ms at %u Hz: %u frames, want %u", rates[i], a, want[i]);
        CHECK(a == (uint32_t)std::max(1.0, std::floor(0.0015 * rates[i] + 0.5)), "%u Hz against round()", rates[i]);
    }
    uint32_t a = 0;
    CHECK(normalize_lookahead(48000, 1, a, err) && a == 1, "asked 1");
    CHECK(normalize_lookahead(48000, 1024, a, err) && a == 1024, "asked 1024");
    return true;
}

static bool check_refusals() {
    std::string err;
    uint32_t a = 0;
    CHECK(!normalize_lookahead(48000, 1025, a, err) && err.find("lookahead_frames") != std::string::npos, "1025 frames: %s", err.c_str());
    CHECK(!normalize_lookahead(1000000, 0, a, err) && err.find("lookahead_frames") != std::string::npos, "1.5 ms at 1 MHz: %s", err.c_str());
    struct Bad {
        const char *word;
        flo_normalize_opts o;
    };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    flo_normalize_opts d = defaults();
    std::vector<Bad> bad;
    auto with = [&](const char *word, auto set) {
        flo_normalize_opts o = d;
        set(o);
        bad.push_back({word, o});
    };
    with("target_lufs", [&](flo_normalize_opts &o) { o.target_lufs = nan; });
    with("target_lufs", [&](flo_normalize_opts &o) { o.target_lufs = INFINITY; });
    with("ceiling_dbtp", [&](flo_normalize_opts &o) { o.ceiling_dbtp = nan; });
    with("ceiling_dbtp", [&](flo_normalize_opts &o) { o.ceiling_dbtp = 61.0; });
    with("ceiling_dbtp", [&](flo_normalize_opts &o) { o.ceiling_dbtp = -61.0; });
    with("max_gain_db", [&](flo_normalize_opts &o) { o.max_gain_db = -1.0; });
    with("max_gain_db", [&](flo_normalize_opts &o) { o.max_gain_db = nan; });
    with("max_gain_db", [&](flo_normalize_opts &o) { o.max_gain_db = 121.0; });
    with("mode", [&](flo_normalize_opts &o) { o.mode = 2; });
    with("lookahead_frames", [&](flo_normalize_opts &o) { o.lookahead_frames = 1025; });
    for (const Bad &b : bad) {
        flo_normalize_opts o;
        err.clear();
        CHECK(!normalize_opts(&b.o, o, err) && err.find(b.word) != std::string::npos, "a bad %s: \"%s\"", b.word, err.c_str());
    }
    flo_normalize_opts o;
    d.mode = FLO_NORM_LIMIT;
    d.lookahead_frames = 1024;
    CHECK(normalize_opts(&d, o, err) && o.mode == FLO_NORM_LIMIT && o.lookahead_frames == 1024, "good options pass through");
    return true;
}

static const uint32_t kLookaheads[] = {1, 12, 72, 576, 1024};

static bool check_cover() {
    for (uint32_t A : {0u, 1u, 12u, 72u, 576u, 1024u}) {
        const uint64_t F = norm_tile_frames(A);
        std::vector<uint64_t> frames = {0, 1, F - 1, F, F + 1, 0, 0, 2 * F + 1, 3 * F + 5, 4 * A + 63, 0};
        std::vector<uint32_t> pre;
        CHECK(clip_tiles(frames.data(), frames.size(), norm_tile_frames(A), pre) && pre.size() == frames.size() + 1 && pre[0] == 0, "A = %u: tiles", A);
        std::vector<std::vector<uint8_t>> hits(frames.size());
        for (size_t i = 0; i < frames.size(); i++) hits[i].assign(frames[i], 0);
        for (uint32_t b = 0; b < pre.back(); b++) {
            // the kernel's search: the last clip whose prefix is at or below b
            size_t lo = 0, hi = frames.size();
            while (hi - lo > 1) {
                const size_t mid = (lo + hi) / 2;
                if (pre[mid] <= b) lo = mid;
                else hi = mid;
            }
            const uint64_t t0 = (uint64_t)(b - pre[lo]) * F;
            CHECK(t0 < frames[lo], "A = %u: tile %u falls on clip %zu, beyond its %llu frames", A, b, lo, (unsigned long long)frames[lo]);
            CHECK(norm_m0(b - pre[lo], A) + (long long)A == (long long)t0 && norm_r0(b - pre[lo], A) + 2ll * A == (long long)t0 &&
                      norm_y0(b - pre[lo], A) + 2ll * A + kNormBefore == (long long)t0,
                  "A = %u: where a tile's planes start", A);
            for (uint64_t f = t0; f < t0 + F && f < frames[lo]; f++) hits[lo][f]++;
        }
        for (size_t i = 0; i < frames.size(); i++)
            for (uint64_t f = 0; f < frames[i]; f++) CHECK(hits[i][f] == 1, "A = %u: frame %llu of clip %zu is made %u times", A, (unsigned long long)f, i, hits[i][f]);
    }
    std::vector<uint64_t> huge = {1ull << 62, 1ull << 62};
    std::vector<uint32_t> pre;
    CHECK(!clip_tiles(huge.data(), huge.size(), norm_tile_frames(72), pre), "more tiles than a launch holds are refused");
    return true;
}

static bool check_reads() {
    CHECK(kNormBefore + kNormAfter + 1 == kNormTaps && norm_span(0) == norm_tile_frames(0) + kNormTaps - 1, "the taps' reach");
    CHECK(norm_lds_bytes(0) / 2 <= 64 * 1024, "the peak kernel's plane fits without asking for more LDS");
    for (uint32_t A : kLookaheads) {
        const uint32_t F = norm_tile_frames(A), lr = norm_r_len(A), lm = norm_m_len(A), span = norm_span(A), w = 2 * A + 1;
        CHECK(F % 4 == 0 && F >= 8 * A, "A = %u: a tile of %u frames starts on 16 bytes and holds eight look-aheads", A, F);
        CHECK(norm_lds_bytes(A) == 2 * 4 * span && norm_lds_bytes(A) <= kNormLdsBytes, "A = %u: %u bytes of LDS", A, norm_lds_bytes(A));
        // the envelope of r's frame f reads staged frames f .. f + 63
        CHECK(lr - 1 + kNormTaps - 1 == span - 1, "A = %u: the last tap of the last frame of p is the last staged frame", A);
        // both planes hold span elements: p, r and the ping-pong of lr elements, m and its prefix sums of lm
        CHECK(lr <= span && lm <= lr, "A = %u: plane lengths", A);
        // the doubling: pw <= w < 2 pw; the last step reads a[i] and a[i + w - pw] for i < lm
        const uint32_t pw = norm_min_pow2(A);
        CHECK((pw & (pw - 1)) == 0 && pw <= w && 2 * pw > w, "A = %u: the power of two %u", A, pw);
        CHECK(lm - 1 + (w - pw) + pw - 1 == lr - 1, "A = %u: the second window of the last m ends at the last r", A);
        // an output j < F sums m[j .. j + 2A], the prefix sums at j - 1 and j + 2A
        CHECK(F - 1 + 2 * A == lm - 1, "A = %u: the last output's window ends at the last m", A);
        // the block-wide prefix sum: odd chunks that cover m
        const uint32_t chunk = norm_scan_chunk(A);
        CHECK((chunk & 1) && (uint64_t)chunk * kNormThreads >= lm && (uint64_t)(chunk - 2) * kNormThreads < lm, "A = %u: chunks of %u", A, chunk);
        // the prefix sums of 12-bit halves stay below 2^32 (each half at most 4096 per element)
        CHECK((uint64_t)lm * 4096 < (1ull << 32), "A = %u: the prefix sums fit 32 bits", A);
        // S fits 64 bits with room, and s <= 2^24
        CHECK((uint64_t)w * kNormUnity / w == kNormUnity, "A = %u: a full window gives unity", A);
    }
    return true;
}

static bool check_bound() {
    const std::vector<float> h = normalize_table();
    CHECK(h.size() == kNormPhases * kNormTaps, "the table has %zu entries", h.size());
    const float B = normalize_skip_bound(h);
    const double want[] = {1.995, 2.124, 2.252, 2.124};
    for (uint32_t q = 0; q < kNormPhases; q++) {
        double s = 0;
        for (uint32_t k = 0; k < kNormTaps; k++) s += std::fabs((double)h[q * kNormTaps + k]);
        CHECK(std::fabs(s - want[q]) < 1e-3, "row %u has l1 norm %.6f", q, s);
        CHECK((double)B >= s * (1.0 + 0x1p-16), "B = %.9g covers row %u", B, q);
    }
    CHECK((double)B < 2.2525 && h[0 * kNormTaps + kNormBefore] > 0.90f && h[0 * kNormTaps + kNormBefore] < 0.92f, "B = %.9g, centre tap %.6f", B,
          h[kNormBefore]);
    return true;
}

int main() {
    if (!check_defaults() || !check_gain() || !check_lookahead() || !check_refusals() || !check_cover() || !check_reads() || !check_bound()) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
