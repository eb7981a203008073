// mix_plan_test.cpp — the host side of the mixing stage (flo_amd/csrc/mix_plan.cpp and the inline mix_part_in_tile of
// mix_plan.hpp that the kernel branches on): that every refusal names its quantity, the fade bound, the two prefixes, and the
// class of a part on every tile against a frame-by-frame restatement for parts that start and end on, one before and one
// after the tile boundaries, fades likewise, and parts that reach past the source's and the output's end.
// Prints "ok <checks>" and returns 0, or names the first case that fails.
// With the argument "dump" it reads lines "n_src start frames at fade_in fade_out T channels" and prints for each
// "F tiles class class ..." (tests/test_mix_model_cpu.py compares them with the model's).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../flo_amd/csrc/clip_tiles.hpp"
#include "../../flo_amd/csrc/mix_plan.hpp"

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

static flo_mix_part part(uint32_t out, uint32_t batch, uint32_t clip, uint64_t start, uint64_t frames, uint64_t at = 0, float gain = 1.f,
                         uint32_t fi = 0, uint32_t fo = 0) {
    flo_mix_part p;
    memset(&p, 0, sizeof p);
    p.out = out;
    p.batch = batch;
    p.clip = clip;
    p.start = start;
    p.frames = frames;
    p.at = at;
    p.gain = gain;
    p.fade_in = fi;
    p.fade_out = fo;
    return p;
}

static MixPart dev_part(const flo_mix_part &g, uint64_t n_src) {
    MixPart p{};
    p.n_src = n_src;
    p.start = g.start;
    p.frames = g.frames;
    p.at = g.at;
    p.fade_in = g.fade_in;
    p.fade_out = g.fade_out;
    p.gain = g.gain;
    return p;
}

struct Sources {
    uint64_t a[2] = {1000, 10}, b[3] = {5, 0, 70};
    int ctx = 0;
    std::vector<MixSource> s;
    Sources() {
        s.resize(2);
        s[0].present = s[1].present = true;
        s[0].ctx = s[1].ctx = &ctx;
        s[0].rate = s[1].rate = 48000;
        s[0].channels = s[1].channels = 2;
        s[0].n_clips = 2;
        s[0].clip_frames = a;
        s[1].n_clips = 3;
        s[1].clip_frames = b;
    }
};

static bool refused(const std::vector<MixSource> &S, const std::vector<uint64_t> &T, const std::vector<flo_mix_part> &parts, const char *word,
                    size_t n_parts = ~(size_t)0) {
    std::vector<uint32_t> ppre, pre;
    std::string err;
    const bool ok = mix_check(S.data(), S.size(), T.size(), T.data(), n_parts == ~(size_t)0 ? parts.size() : n_parts, parts.data(), ppre, pre, err);
    CHECK(!ok, "expected a refusal that names %s", word);
    CHECK(err.find(word) != std::string::npos, "the refusal \"%s\" does not name %s", err.c_str(), word);
    return true;
}

static bool check_refusals() {
    Sources src;
    const std::vector<MixSource> &S = src.s;
    std::vector<uint32_t> ppre, pre;
    std::string err;
    const uint32_t F = edit_tile_frames(2);
    const std::vector<uint64_t> T = {100, 0, 2 * (uint64_t)F + 1, 7};
    const std::vector<flo_mix_part> good = {part(0, 0, 0, 5, 100, 3, 0.5f, 100, 100), part(0, 1, 2, 50, 200, 90, -1.f), part(0, 0, 0, 5, 100, 3),
                                            part(2, 0, 1, 0, 0), part(3, 1, 1, 9, 4, 1000, 0.f)};
    CHECK(mix_check(S.data(), 2, T.size(), T.data(), good.size(), good.data(), ppre, pre, err), "a good list is refused: %s", err.c_str());
    CHECK(ppre == (std::vector<uint32_t>{0, 3, 3, 4, 5}), "the prefix of parts");
    CHECK(pre == (std::vector<uint32_t>{0, 1, 1, 4, 5}), "the prefix of tiles");
    CHECK(mix_check(S.data(), 2, 0, nullptr, 0, nullptr, ppre, pre, err) && ppre == std::vector<uint32_t>{0} && pre == std::vector<uint32_t>{0},
          "no outputs: %s", err.c_str());
    CHECK(mix_check(S.data(), 1, T.size(), T.data(), 0, nullptr, ppre, pre, err) && ppre == std::vector<uint32_t>(5, 0), "no parts: %s", err.c_str());
    if (!refused({}, T, {}, "n_srcs")) return false;
    std::vector<MixSource> bad = S;
    bad[1].present = false;
    if (!refused(bad, T, good, "source 1 is NULL")) return false;
    bad = S;
    int other = 0;
    bad[1].ctx = &other;
    if (!refused(bad, T, good, "context")) return false;
    bad = S;
    bad[1].rate = 44100;
    if (!refused(bad, T, good, "sample_rate")) return false;
    bad = S;
    bad[1].channels = 1;
    if (!refused(bad, T, good, "channels")) return false;
    if (!refused(S, T, {part(4, 0, 0, 0, 1)}, "out 4")) return false;
    if (!refused(S, T, {part(2, 0, 0, 0, 1), part(1, 0, 0, 0, 1)}, "out must not decrease")) return false;
    if (!refused(S, T, {part(0, 2, 0, 0, 1)}, "batch")) return false;
    if (!refused(S, T, {part(0, 0, 2, 0, 1)}, "clip")) return false;
    if (!refused(S, T, {part(0, 1, 3, 0, 1)}, "clip")) return false;
    if (!refused(S, T, {part(0, 0, 0, 0, 10, 0, 1.f, 11, 0)}, "fade_in")) return false;
    if (!refused(S, T, {part(0, 0, 0, 0, 10, 0, 1.f, 0, 11)}, "fade_out")) return false;
    if (!refused(S, T, {part(0, 0, 0, 0, 1ull << 24, 0, 1.f, 1u << 24, 0)}, "fade_in")) return false;
    if (!refused(S, T, {part(0, 0, 0, 0, 1ull << 24, 0, 1.f, 0, 1u << 24)}, "fade_out")) return false;
    const flo_mix_part longest = part(0, 0, 0, 0, (1ull << 24) - 1, 0, 1.f, (1u << 24) - 1, (1u << 24) - 1);
    CHECK(mix_check(S.data(), 2, T.size(), T.data(), 1, &longest, ppre, pre, err), "fades of 2^24 - 1 are refused: %s", err.c_str());
    if (!refused(S, T, {part(0, 0, 0, 0, 1, 0, std::numeric_limits<float>::quiet_NaN())}, "gain")) return false;
    if (!refused(S, T, {part(0, 0, 0, 0, 1, 0, std::numeric_limits<float>::infinity())}, "gain")) return false;
    if (!refused(S, T, {part(0, 0, 0, 0, ~0ull - 2, 3)}, "at + frames")) return false;
    if (!refused(S, T, {part(0, 0, 0, 5, ~0ull - 4, 0)}, "start + frames")) return false;
    const flo_mix_part edge = part(0, 0, 0, 5, ~0ull - 5, 5);
    CHECK(mix_check(S.data(), 2, T.size(), T.data(), 1, &edge, ppre, pre, err), "sums of 2^64 - 1 are refused: %s", err.c_str());
    if (sizeof(size_t) > 4 && !refused(S, T, good, "n_parts", (size_t)1 << 32)) return false;
    const uint64_t most = (uint64_t)(SIZE_MAX / 8) / 2;
    if (!refused(S, {5, most + 1}, {}, "out_frames")) return false;
    if (!refused(S, {5, 0x7FFFFFFFull * F, 1}, {}, "tiles")) return false;
    CHECK(mix_check(S.data(), 2, 1, &(const uint64_t &)(0x7FFFFFFFull * F), 0, nullptr, ppre, pre, err) && pre[1] == 0x7FFFFFFFu, "2^31 - 1 tiles: %s", err.c_str());
    std::vector<uint32_t> a, b;
    CHECK(!mix_check(S.data(), 2, 1, nullptr, 0, nullptr, a, b, err) && err.find("out_frames") != std::string::npos, "a NULL out_frames");
    CHECK(!mix_check(S.data(), 2, T.size(), T.data(), 1, nullptr, a, b, err) && err.find("parts") != std::string::npos, "a NULL parts");
    return true;
}

// the class of a part on the tile [t0, t0 + nf), frame by frame
static uint32_t slow_class(const MixPart &p, uint64_t T, uint64_t t0, uint32_t nf) {
    uint32_t live = 0, faded = 0;
    for (uint64_t t = t0; t < t0 + nf; t++) {
        if (t < p.at || t - p.at >= p.frames || t >= T) continue;
        const uint64_t u = t - p.at;
        if (p.start >= p.n_src || u >= p.n_src - p.start) continue;
        live++;
        if (u < p.fade_in || p.frames - 1 - u < p.fade_out) faded++;
    }
    return !live ? kMixNone : live == nf && !faded ? kMixWhole : kMixPartial;
}

static bool check_classes() {
    long n = 0, seen[3] = {0, 0, 0};
    for (uint32_t c : {2u, 3u}) {
        const uint32_t F = edit_tile_frames(c);
        const uint64_t N = 3 * (uint64_t)F + 5;
        const uint32_t around[] = {0, 1, 2, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1};
        for (uint64_t at : around)
            for (uint64_t T : {(uint64_t)1, (uint64_t)F, (uint64_t)F + 1, 2 * (uint64_t)F - 1, 3 * (uint64_t)F, 3 * (uint64_t)F + 5})
                for (uint64_t frames : {(uint64_t)0, (uint64_t)1, (uint64_t)F - 1, (uint64_t)F, (uint64_t)F + 1, 2 * (uint64_t)F + 5})
                    for (uint32_t fi : around)
                        for (uint32_t fo : around) {
                            if (fi > frames || fo > frames) continue;
                            for (uint64_t start : {(uint64_t)0, (uint64_t)3, N - F, N - 1, N, N + 5}) {
                                const MixPart p = dev_part(part(0, 0, 0, start, frames, at, 1.f, fi, fo), N);
                                for (uint64_t t0 = 0; t0 < T; t0 += F) {
                                    const uint32_t nf = T - t0 < F ? (uint32_t)(T - t0) : F;
                                    const uint32_t got = mix_part_in_tile(p, T, t0, nf), want = slow_class(p, T, t0, nf);
                                    CHECK(got == want, "class %u, not %u: tile at %llu of %u, T %llu, F %u, start %llu, frames %llu, at %llu, fades %u %u", got, want,
                                          (unsigned long long)t0, nf, (unsigned long long)T, F, (unsigned long long)start, (unsigned long long)frames,
                                          (unsigned long long)at, fi, fo);
                                    seen[got]++;
                                    n++;
                                }
                            }
                        }
    }
    CHECK(n > 100000 && seen[kMixNone] > 1000 && seen[kMixWhole] > 1000 && seen[kMixPartial] > 1000, "only %ld tiles were classified (%ld none, %ld whole, %ld partial)", n,
          seen[0], seen[1], seen[2]);
    // a part that starts past the source, one whose start is the largest integer, one that lies wholly past the output
    const MixPart far = dev_part(part(0, 0, 0, ~0ull - 5000, 5000), 100);
    CHECK(mix_avail(far) == 0 && mix_part_in_tile(far, 9000, 0, 2048) == kMixNone, "a part past the source");
    const MixPart reach = dev_part(part(0, 0, 0, 90, 5000), 100);
    CHECK(mix_avail(reach) == 10 && mix_part_in_tile(reach, 9000, 0, 2048) == kMixPartial && mix_part_in_tile(reach, 9000, 2048, 2048) == kMixNone,
          "a part that reaches past the source");
    const MixPart late = dev_part(part(0, 0, 0, 0, 100, ~0ull - 100), 100);
    CHECK(mix_part_in_tile(late, 4096, 2048, 2048) == kMixNone, "a part past the output");
    const MixPart cut = dev_part(part(0, 0, 0, 0, 5000, 2048), 5000);
    CHECK(mix_part_in_tile(cut, 4000, 2048, 4000 - 2048) == kMixWhole && mix_part_in_tile(cut, 4000, 0, 2048) == kMixNone, "a part cut by the output's end");
    return true;
}

static int dump() {
    unsigned long long n_src, start, frames, at, T;
    unsigned fi, fo, ch;
    while (scanf("%llu %llu %llu %llu %u %u %llu %u", &n_src, &start, &frames, &at, &fi, &fo, &T, &ch) == 8) {
        const MixPart p = dev_part(part(0, 0, 0, start, frames, at, 1.f, fi, fo), n_src);
        const uint32_t F = edit_tile_frames(ch);
        const uint64_t frames_out = T;
        std::vector<uint32_t> pre;
        if (!clip_tiles(&frames_out, 1, F, pre)) return 1;
        printf("%u %u", F, pre[1]);
        for (uint32_t k = 0; k < pre[1]; k++) {
            const uint64_t t0 = (uint64_t)k * F;
            printf(" %u", mix_part_in_tile(p, T, t0, T - t0 < F ? (uint32_t)(T - t0) : F));
        }
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "dump")) return dump();
    if (!check_refusals() || !check_classes()) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
