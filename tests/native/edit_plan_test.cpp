// edit_plan_test.cpp — the host side of the batch editing stage (flo_amd/csrc/edit_plan.cpp and the inline tile geometry of
// edit_plan.hpp that the kernel shares): that every refusal names its quantity, the tile prefixes, and the class of every tile
// against a frame-by-frame restatement for cuts, pads and fades placed on, one before and one after the tile boundaries and
// for cuts that reach past the source. Prints "ok <checks>" and returns 0, or names the first case that fails.
// With the argument "dump" it reads lines "n_src start frames pad_head pad_tail fade_in fade_out out_channels" and prints for
// each "F tiles class class ..." (tests/test_edit_model_cpu.py compares them with the model's).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../flo_amd/csrc/clip_tiles.hpp"
#include "../../flo_amd/csrc/edit_plan.hpp"

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

static flo_edit_segment seg(uint32_t clip, uint64_t start, uint64_t frames, uint32_t ph = 0, uint32_t pt = 0, uint32_t fi = 0, uint32_t fo = 0) {
    flo_edit_segment s;
    memset(&s, 0, sizeof s);
    s.clip = clip;
    s.start = start;
    s.frames = frames;
    s.pad_head = ph;
    s.pad_tail = pt;
    s.fade_in = fi;
    s.fade_out = fo;
    return s;
}

static EditSeg dev_seg(const flo_edit_segment &g, uint64_t n_src) {
    EditSeg s{};
    s.n_src = n_src;
    s.start = g.start;
    s.frames = g.frames;
    s.pad_head = g.pad_head;
    s.pad_tail = g.pad_tail;
    s.fade_in = g.fade_in;
    s.fade_out = g.fade_out;
    return s;
}

static bool refused(const EditSource &S, const std::vector<flo_edit_segment> &segs, uint32_t cout, const float *matrix, const char *word) {
    std::vector<uint64_t> T;
    std::string err;
    const bool ok = edit_check(S, segs.size(), segs.data(), cout, matrix, T, err);
    CHECK(!ok, "expected a refusal that names %s", word);
    CHECK(err.find(word) != std::string::npos, "the refusal \"%s\" does not name %s", err.c_str(), word);
    return true;
}

static bool check_refusals() {
    const uint64_t frames[2] = {1000, 10};
    EditSource S;
    S.n_clips = 2;
    S.clip_frames = frames;
    S.channels = 2;
    const float m21[2] = {0.5f, 0.5f};
    std::vector<uint64_t> T;
    std::string err;
    std::vector<flo_edit_segment> good = {seg(0, 5, 100, 3, 4, 100, 100), seg(1, 50, 20), seg(1, 0, 0)};
    CHECK(edit_check(S, good.size(), good.data(), 2, nullptr, T, err), "a good list is refused: %s", err.c_str());
    CHECK(T.size() == 3 && T[0] == 107 && T[1] == 20 && T[2] == 0, "T of the good list");
    CHECK(edit_check(S, good.size(), good.data(), 1, m21, T, err), "a good 2 -> 1 mix is refused: %s", err.c_str());
    CHECK(edit_check(S, 0, nullptr, 2, nullptr, T, err) && T.empty(), "no segments: %s", err.c_str());
    if (!refused(S, {seg(2, 0, 1)}, 2, nullptr, "clip")) return false;
    flo_edit_segment r = seg(0, 0, 1);
    r.reserved = 7;
    if (!refused(S, {good[0], r}, 2, nullptr, "reserved")) return false;
    if (!refused(S, {seg(0, 0, 10, 0, 0, 11, 0)}, 2, nullptr, "fade_in")) return false;
    if (!refused(S, {seg(0, 0, 10, 0, 0, 0, 11)}, 2, nullptr, "fade_out")) return false;
    if (!refused(S, {seg(0, 0, 1ull << 24, 0, 0, 1u << 24, 0)}, 2, nullptr, "fade_in")) return false;
    if (!refused(S, {seg(0, 0, 1ull << 24, 0, 0, 0, 1u << 24)}, 2, nullptr, "fade_out")) return false;
    CHECK(edit_check(S, 1, &(const flo_edit_segment &)seg(0, 0, 1ull << 24, 0, 0, (1u << 24) - 1, (1u << 24) - 1), 2, nullptr, T, err),
          "fades of 2^24 - 1 are refused: %s", err.c_str());
    if (!refused(S, good, 1, nullptr, "matrix")) return false;
    const float nanm[2] = {0.5f, std::numeric_limits<float>::quiet_NaN()}, infm[2] = {std::numeric_limits<float>::infinity(), 0.f};
    if (!refused(S, good, 1, nanm, "matrix")) return false;
    if (!refused(S, good, 1, infm, "matrix")) return false;
    std::vector<float> big(9 * 9, 0.25f);
    if (!refused(S, good, 9, big.data(), "out_channels")) return false;
    EditSource S9 = S;
    S9.channels = 9;
    if (!refused(S9, good, 2, big.data(), "in_channels")) return false;
    CHECK(edit_check(S9, good.size(), good.data(), 9, nullptr, T, err), "a lossless copy of 9 channels is refused: %s", err.c_str());
    S9.lossy = true;
    if (!refused(S9, good, 9, nullptr, "out_channels")) return false;
    if (!refused(S, good, 0, nullptr, "out_channels")) return false;
    const uint64_t most = (uint64_t)(SIZE_MAX / 8) / 2;
    if (!refused(S, {seg(0, 0, most + 1)}, 2, nullptr, "frames")) return false;
    if (!refused(S, {seg(0, 0, most, 1, 0)}, 2, nullptr, "frames")) return false;
    if (!refused(S, {seg(0, 0, most - 1, 1, 1)}, 2, nullptr, "frames")) return false;
    CHECK(edit_check(S, 1, &(const flo_edit_segment &)seg(0, ~0ull, most - 2, 1, 1), 2, nullptr, T, err) && T[0] == most,
          "the largest T is refused: %s", err.c_str());
    CHECK(!edit_threshold(-1e-30f, err) && err.find("threshold") != std::string::npos, "a negative threshold");
    CHECK(!edit_threshold(std::numeric_limits<float>::quiet_NaN(), err) && err.find("threshold") != std::string::npos, "a NaN threshold");
    CHECK(edit_threshold(0.f, err) && edit_threshold(-0.f, err) && edit_threshold(std::numeric_limits<float>::infinity(), err), "0 and +inf are thresholds");
    return true;
}

// the class of a tile frame by frame
static uint32_t slow_class(const EditSeg &s, uint64_t tile, uint32_t F) {
    const uint64_t T = edit_out_frames(s);
    uint32_t cls = 0;
    for (uint64_t t = tile * F; t < tile * F + F && t < T; t++) {
        if (t < s.pad_head || t - s.pad_head >= s.frames) {
            cls |= kEditEdge;
            continue;
        }
        const uint64_t u = t - s.pad_head;
        if (s.start >= s.n_src || u >= s.n_src - s.start) cls |= kEditEdge;
        if (u < s.fade_in || s.frames - 1 - u < s.fade_out) cls |= kEditFaded;
    }
    return cls;
}

static bool check_geometry() {
    for (uint32_t c = 1; c <= 255; c++) {
        const uint32_t F = edit_tile_frames(c);
        CHECK(F >= 16 && F % 4 == 0 && (uint64_t)F * c <= kEditTileFloats && (uint64_t)(F + 4) * c > kEditTileFloats, "tile frames of %u channels: %u", c, F);
    }
    CHECK(edit_tile_frames(1) == 4096 && edit_tile_frames(2) == 2048 && edit_tile_frames(3) == 1364 && edit_tile_frames(8) == 512, "the tiles of 1, 2, 3 and 8 channels");
    for (uint32_t c : {1u, 2u, 3u, 8u}) {
        const uint32_t F = edit_tile_frames(c);
        const uint64_t lens[] = {0, 1, F - 1, F, F + 1, 2 * (uint64_t)F + 5};
        const uint32_t want[] = {0, 1, 1, 1, 2, 3};
        std::vector<uint32_t> pre;
        CHECK(clip_tiles(lens, 6, F, pre) && pre.size() == 7, "the prefix of six clips");
        uint32_t t = 0;
        for (int i = 0; i < 6; i++) {
            CHECK(pre[i] == t, "pre[%d] of %u channels is %u, not %u", i, c, pre[i], t);
            t += want[i];
        }
        CHECK(pre[6] == t, "the tiles in all");
        // whole clips without pads or fades: every tile interior
        for (uint64_t n : lens)
            for (uint64_t k = 0; k * F < n; k++) {
                const EditSeg s = dev_seg(seg(0, 0, n), n);
                CHECK(edit_tile_class(s, k, F) == kEditInterior, "tile %llu of a whole clip of %llu frames is not interior", (unsigned long long)k, (unsigned long long)n);
            }
    }
    const uint64_t huge[2] = {0x7FFFFFFFull * 16, 17};
    std::vector<uint32_t> pre;
    CHECK(!clip_tiles(huge, 2, 16, pre), "more than 2^31 - 1 tiles are refused");
    CHECK(clip_tiles(huge, 1, 16, pre) && pre[1] == 0x7FFFFFFFu, "2^31 - 1 tiles are accepted");
    return true;
}

static bool check_classes() {
    long n = 0;
    for (uint32_t c : {2u, 3u}) {
        const uint32_t F = edit_tile_frames(c);
        const uint64_t N = 3 * (uint64_t)F + 5;
        const uint32_t around[] = {0, 1, 2, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1};
        for (uint32_t ph : around)
            for (uint32_t pt : {0u, 1u, F})
                for (uint64_t frames : {(uint64_t)0, (uint64_t)1, (uint64_t)F - 1, (uint64_t)F, (uint64_t)F + 1, 2 * (uint64_t)F + 5})
                    for (uint32_t fi : around)
                        for (uint32_t fo : around) {
                            if (fi > frames || fo > frames) continue;
                            for (uint64_t start : {(uint64_t)0, (uint64_t)3, N - F, N - 1, N, N + 5}) {
                                const EditSeg s = dev_seg(seg(0, start, frames, ph, pt, fi, fo), N);
                                const uint64_t T = edit_out_frames(s);
                                for (uint64_t k = 0; k * F < T; k++) {
                                    const uint32_t got = edit_tile_class(s, k, F), want = slow_class(s, k, F);
                                    CHECK(got == want, "class %u, not %u: tile %llu, F %u, start %llu, frames %llu, pads %u %u, fades %u %u", got, want,
                                          (unsigned long long)k, F, (unsigned long long)start, (unsigned long long)frames, ph, pt, fi, fo);
                                    n++;
                                }
                            }
                        }
    }
    CHECK(n > 100000, "only %ld tiles were classified", n);
    // a cut that starts past the source, and one whose start is the largest integer: every tile an edge
    const EditSeg far = dev_seg(seg(0, ~0ull, 5000), 100);
    CHECK(edit_avail(far) == 0 && edit_tile_class(far, 0, 2048) == kEditEdge && edit_tile_class(far, 2, 2048) == kEditEdge, "a cut past the source");
    const EditSeg part = dev_seg(seg(0, 90, 5000), 100);
    CHECK(edit_avail(part) == 10 && edit_tile_class(part, 0, 2048) == kEditEdge, "a cut that reaches past the source");
    float rows[kEditMaxMix * kEditMaxMix];
    const float m[6] = {1, 2, 3, 4, 5, 6};
    edit_matrix_rows(m, 3, 2, rows);
    CHECK(rows[0] == 1 && rows[2] == 3 && rows[3] == 0 && rows[8] == 4 && rows[10] == 6 && rows[11] == 0 && rows[16] == 0, "the matrix in rows of 8");
    return true;
}

static int dump() {
    unsigned long long n_src, start, frames;
    unsigned ph, pt, fi, fo, cout;
    while (scanf("%llu %llu %llu %u %u %u %u %u", &n_src, &start, &frames, &ph, &pt, &fi, &fo, &cout) == 8) {
        const EditSeg s = dev_seg(seg(0, start, frames, ph, pt, fi, fo), n_src);
        const uint32_t F = edit_tile_frames(cout);
        const uint64_t T = edit_out_frames(s);
        std::vector<uint32_t> pre;
        if (!clip_tiles(&T, 1, F, pre)) return 1;
        printf("%u %u", F, pre[1]);
        for (uint32_t k = 0; k < pre[1]; k++) printf(" %u", edit_tile_class(s, k, F));
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "dump")) return dump();
    if (!check_refusals() || !check_geometry() || !check_classes()) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
