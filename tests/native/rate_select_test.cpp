// rate_select_test.cpp — the candidate choice of the rate-targeted encode (flo_amd/csrc/rate_select.cpp) on the host.
// Prints "ok <checks>" and returns 0, or names the first case that fails.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../flo_amd/csrc/rate_select.hpp"

using flo::rate_pick;
using flo::RatePick;

static int g_checks = 0;
static bool expect(const char *what, const std::vector<float> &q, const std::vector<uint64_t> &z, uint64_t budget, uint32_t index, int fits) {
    const RatePick p = rate_pick(q.size(), q.data(), z.data(), budget);
    g_checks++;
    if (p.index == index && p.fits == fits) return true;
    fprintf(stderr, "%s: budget %llu -> (%u, %d), expected (%u, %d)\n", what, (unsigned long long)budget, p.index, p.fits, index, fits);
    return false;
}

int main() {
    bool ok = true;
    // the table the Python test sends through flo_rate_pick as well (tests/test_rate_select_cpu.py): unsorted qualities with a
    // duplicate, sizes that do not grow with quality
    const std::vector<float> q = {0.5f, 0.125f, 0.75f, 0.5f, 0.25f, 1.0f};
    const std::vector<uint64_t> z = {500, 300, 450, 480, 700, 900};
    ok &= expect("everything fits: largest quality", q, z, 1000, 5, 1);
    ok &= expect("exactly equal fits", q, z, 900, 5, 1);
    ok &= expect("one below: next quality down", q, z, 899, 2, 1);
    // 0.75 (450 bytes) wins although 0.25 is bigger (700) and does not fit, and 0.5 is bigger (500, 480) too
    ok &= expect("non-monotone: largest fitting quality", q, z, 460, 2, 1);
    ok &= expect("duplicates: the one that fits", q, z, 449, 1, 1);
    ok &= expect("duplicates both fit: lower index", {0.5f, 0.5f, 0.25f}, {10, 10, 5}, 10, 0, 1);
    ok &= expect("duplicates, only the second fits", {0.5f, 0.5f, 0.25f}, {11, 10, 5}, 10, 1, 1);
    ok &= expect("equal to the smallest", q, z, 300, 1, 1);
    ok &= expect("nothing fits: lowest quality", q, z, 299, 1, 0);
    ok &= expect("nothing fits, budget 0", q, z, 0, 1, 0);
    ok &= expect("nothing fits, lowest quality twice: lower index", {0.5f, 0.0f, 0.0f}, {9, 8, 7}, 1, 1, 0);
    // K = 1
    ok &= expect("one candidate fits", {0.3f}, {100}, 100, 0, 1);
    ok &= expect("one candidate does not", {0.3f}, {100}, 99, 0, 0);
    // K = 32: qualities descending, sizes descending; budget between two neighbours
    {
        std::vector<float> q32(32);
        std::vector<uint64_t> z32(32);
        for (int i = 0; i < 32; i++) {
            q32[i] = (float)(31 - i) / 31.0f;
            z32[i] = 1000 * (uint64_t)(32 - i);
        }
        ok &= expect("32 candidates, all fit", q32, z32, 32000, 0, 1);
        ok &= expect("32 candidates, middle", q32, z32, 16500, 16, 1);
        ok &= expect("32 candidates, last only", q32, z32, 1000, 31, 1);
        ok &= expect("32 candidates, none", q32, z32, 999, 31, 0);
    }
    // clamping as the encoder clamps: NaN -> 0, below 0 -> 0, above 1 -> 1
    ok &= expect("NaN counts as 0: not the largest", {NAN, 0.1f}, {5, 5}, 5, 1, 1);
    ok &= expect("NaN counts as 0: the lowest", {0.1f, NAN}, {50, 60}, 5, 1, 0);
    ok &= expect("NaN and 0 tie: lower index", {0.0f, NAN, 0.2f}, {5, 5, 50}, 5, 0, 1);
    ok &= expect("2.0 clamps to 1.0: ties with 1.0, lower index", {1.0f, 2.0f}, {5, 5}, 5, 0, 1);
    ok &= expect("2.0 clamps to 1.0: beats 0.9", {0.9f, 2.0f}, {5, 5}, 5, 1, 1);
    ok &= expect("-1 clamps to 0: ties with 0, lower index", {0.0f, -1.0f}, {50, 50}, 5, 0, 0);
    ok &= expect("-1 clamps to 0: below 0.1", {0.1f, -1.0f}, {50, 50}, 5, 1, 0);
    ok &= expect("huge sizes", {0.1f, 0.2f}, {UINT64_MAX, UINT64_MAX - 1}, UINT64_MAX - 1, 1, 1);
    g_checks += 3;
    ok &= flo::rate_clamp_quality(NAN) == 0.0f && flo::rate_clamp_quality(-0.5f) == 0.0f && flo::rate_clamp_quality(1.5f) == 1.0f &&
          flo::rate_clamp_quality(0.4f) == 0.4f;
    if (!ok) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
