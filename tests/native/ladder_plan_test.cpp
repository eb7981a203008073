// ladder_plan_test.cpp — the partition of a batch's clips into groups for the passes over candidate qualities, and the
// scratch per frame that sizes the groups (flo_amd/csrc/ladder_plan.cpp) on the host. (The layout of the files:
// file_layout_test.cpp.) Prints "ok <checks>" and returns 0, or names the first case that fails.
#include <cstdio>
#include <vector>

#include "../../flo_amd/csrc/ladder_plan.hpp"

using flo::ClipGroup;

static int g_checks = 0;

// every clip in exactly one group, in order; a group stays under the limit unless it holds one clip; the group's frame
// count and longest clip are what its clips say; `want` = the expected clips per group
static bool expect(const char *what, const std::vector<uint32_t> &hops, uint64_t per_frame, uint64_t limit, const std::vector<size_t> &want) {
    const std::vector<ClipGroup> g = flo::partition_clips(hops.data(), hops.size(), per_frame, limit);
    g_checks++;
    bool ok = g.size() == want.size();
    const uint64_t cap = per_frame ? limit / per_frame : UINT64_MAX;   // frames * per_frame <= limit, without the product
    size_t next = 0;
    for (size_t k = 0; ok && k < g.size(); k++) {
        ok = g[k].first == next && g[k].count == want[k] && g[k].count >= 1;
        uint64_t frames = 0;
        uint32_t longest = 0;
        for (size_t i = 0; ok && i < g[k].count; i++) {
            frames += hops[next + i];
            longest = hops[next + i] > longest ? hops[next + i] : longest;
        }
        ok = ok && frames == g[k].frames && longest == g[k].max_hops;
        ok = ok && (g[k].count == 1 || frames <= cap);
        // greedy: the next clip would not have fitted
        if (ok && k + 1 < g.size()) ok = frames + hops[next + g[k].count] > cap;
        next += g[k].count;
    }
    ok = ok && next == hops.size();
    if (!ok) {
        fprintf(stderr, "%s: groups", what);
        for (const ClipGroup &x : g) fprintf(stderr, " [%zu +%zu: %llu frames]", x.first, x.count, (unsigned long long)x.frames);
        fprintf(stderr, "\n");
    }
    return ok;
}

int main() {
    bool ok = true;
    const std::vector<uint32_t> hops = {2, 6, 45, 4, 10, 2, 21};
    ok &= expect("everything fits: one group", hops, 100, 100 * 90, {7});
    ok &= expect("exactly fitting", hops, 100, 100 * 8, {2, 1, 1, 1, 1, 1});     // 2 + 6 = 8 fits exactly; 45 and 10 alone
    ok &= expect("one frame short of fitting", hops, 100, 100 * 8 - 1, {1, 1, 1, 1, 1, 1, 1});
    ok &= expect("limit below the smallest clip: one clip per group", hops, 100, 150, {1, 1, 1, 1, 1, 1, 1});
    ok &= expect("limit of one byte", hops, 100, 1, {1, 1, 1, 1, 1, 1, 1});
    ok &= expect("an oversized clip between groups", hops, 100, 100 * 26, {2, 1, 3, 1});
    ok &= expect("one clip", {5}, 100, 100 * 5, {1});
    ok &= expect("one clip above the limit", {5}, 100, 100, {1});
    ok &= expect("no clips", {}, 100, 1000, {});
    // empty clips (one frame each: a clip of no samples still has its priming frame) between longer ones
    ok &= expect("empty clips", {1, 1, 9, 1, 1, 1, 9, 1}, 10, 10 * 10, {2, 2, 2, 2});
    ok &= expect("all empty", {1, 1, 1, 1, 1}, 10, 10 * 2, {2, 2, 1});
    // sizes that would overflow a product in 64 bits
    ok &= expect("huge bytes per frame", {3, 3}, UINT64_MAX / 4, UINT64_MAX, {1, 1});
    ok &= expect("huge limit", {4000000000u, 4000000000u}, 1u << 20, UINT64_MAX, {2});
    ok &= expect("bytes per frame of 0", {7, 7}, 0, 0, {2});

    // scratch per frame: K slots + K frame sizes and offsets + the level rows (three for stereo, whose pass 1 leaves the band maxima)
    g_checks += 3;
    ok &= flo::ladder_frame_bytes(2, 16, 4352) == 16 * (4352 + 12) + 2 * 128 * 3;
    ok &= flo::ladder_frame_bytes(1, 1, 4352) == 4352 + 12 + 128 * 2;
    ok &= flo::ladder_frame_bytes(8, 32, 17040) == 32ull * (17040 + 12) + 8 * 128 * 2;

    // the level rows alone (all the scratch of a size curve's frame); 26 stereo frames fit into 20 KiB, 27 do not (the group
    // sizes tests/test_gpu_rate.py's test_groups_of_clips_give_the_same_array counts on)
    g_checks += 3;
    ok &= flo::level_row_bytes(2) == 768 && flo::level_row_bytes(1) == 256;
    ok &= flo::level_row_bytes(2) * 26 <= 20 * 1024 && 20 * 1024 < flo::level_row_bytes(2) * 27;
    ok &= flo::ladder_frame_bytes(2, 16, 4352) == 16 * (4352 + 12) + flo::level_row_bytes(2);
    if (!ok) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
