// clip_tiles_test.cpp — the flat (clip, tile) work list every batch-to-batch operation shares (flo_amd/csrc/clip_tiles.hpp):
// the prefix at and around a tile's size and at the edge of what a launch holds, the lookup a workgroup makes (run here on
// the host) for lists with empty clips in every position, and the block layout's alignment. Prints "ok <checks>" and
// returns 0, or names the first case that fails.
#include <cstdio>
#include <vector>

#include "../../flo_amd/csrc/clip_tiles.hpp"

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

static bool check_prefix() {
    std::vector<uint32_t> pre;
    for (uint64_t F : {1ull, 2ull, 16ull, 2048ull, 4096ull, 0xFFFFFFFFull}) {
        const uint64_t count[] = {0, F - 1, F, F + 1, 0, 0, 3 * F + 1, 0};
        const uint32_t want[] = {0, F > 1 ? 1u : 0u, 1, 2, 0, 0, 4, 0};
        CHECK(clip_tiles(count, 8, F, pre), "tiles of %llu: refused", (unsigned long long)F);
        CHECK(pre.size() == 9 && pre[0] == 0, "tiles of %llu: %zu entries from %u", (unsigned long long)F, pre.size(), pre[0]);
        uint32_t t = 0;
        for (int i = 0; i < 8; i++) {
            CHECK(pre[i] == t, "tiles of %llu: pre[%d] is %u, not %u", (unsigned long long)F, i, pre[i], t);
            t += want[i];
        }
        CHECK(pre[8] == t, "tiles of %llu: %u in all, not %u", (unsigned long long)F, pre[8], t);
    }
    pre.assign(3, 7);
    CHECK(clip_tiles(nullptr, 0, 16, pre) && pre.size() == 1 && pre[0] == 0, "no clips: pre is {0}");
    // the most a launch holds, reached in one clip and across two, and one tile more
    const uint64_t most = 0x7FFFFFFFull;
    const uint64_t one[] = {most * 16}, split[] = {most * 16 - 16, 0, 1}, over[] = {most * 16, 0, 1}, over1[] = {most * 16 + 1};
    CHECK(clip_tiles(one, 1, 16, pre) && pre[1] == most, "2^31 - 1 tiles of one clip are accepted");
    CHECK(clip_tiles(split, 3, 16, pre) && pre[3] == most && pre[2] == most - 1, "2^31 - 1 tiles of two clips are accepted");
    CHECK(!clip_tiles(over, 3, 16, pre), "2^31 tiles of two clips are refused");
    CHECK(!clip_tiles(over1, 1, 16, pre), "2^31 tiles of one clip are refused");
    // counts whose rounding up would wrap
    const uint64_t top[] = {~0ull}, after[] = {1, ~0ull};
    CHECK(!clip_tiles(top, 1, 2, pre), "2^64 - 1 items in tiles of 2 are refused");
    CHECK(!clip_tiles(top, 1, 1, pre) && !clip_tiles(after, 2, 1, pre), "2^64 - 1 items in tiles of 1 are refused, behind another clip too");
    CHECK(clip_tiles(top, 1, ~0ull, pre) && pre[1] == 1, "2^64 - 1 items are one tile of 2^64 - 1");
    CHECK(!clip_tiles(nullptr, (size_t)0x80000000ull, 16, pre), "2^31 clips are refused (before the list is read)");
    return true;
}

// every b in [0, pre[n]) maps to the one clip k with pre[k] <= b < pre[k + 1]
static bool check_lookup() {
    const std::vector<std::vector<uint64_t>> lists = {
        {1},          {33},           {0, 5},          {0, 0, 0, 5},       {5, 0},       {5, 0, 0, 0},    {3, 0, 4},
        {3, 0, 0, 4}, {0, 1, 0, 1, 0}, {16, 16, 16, 16}, {1, 0, 0, 0, 0, 0, 1}, {0, 0, 40, 0, 0, 17, 0, 0, 1, 0}, {15, 17, 0, 16, 1, 0, 0, 32, 31},
    };
    for (size_t l = 0; l < lists.size(); l++)
        for (uint64_t F : {1ull, 16ull}) {
            const std::vector<uint64_t> &count = lists[l];
            const unsigned n = (unsigned)count.size();
            std::vector<uint32_t> pre;
            CHECK(clip_tiles(count.data(), n, F, pre), "list %zu: refused", l);
            CHECK(pre[n] > 0, "list %zu has no tiles", l);
            for (unsigned b = 0; b < pre[n]; b++) {
                const unsigned k = tile_clip(pre.data(), n, b);
                CHECK(k < n, "list %zu, tiles of %llu: tile %u maps to clip %u of %u", l, (unsigned long long)F, b, k, n);
                CHECK(pre[k] <= b && b < pre[k + 1], "list %zu, tiles of %llu: tile %u maps to clip %u, which holds [%u, %u)", l, (unsigned long long)F, b,
                      k, pre[k], pre[k + 1]);
                CHECK(count[k] > 0, "list %zu, tiles of %llu: tile %u maps to the empty clip %u", l, (unsigned long long)F, b, k);
            }
        }
    return true;
}

static bool check_layout() {
    BlockLayout B;
    const size_t a = B.take(5), b = B.take(0), c = B.take(16), d = B.take(17);
    CHECK(a == 0 && b == 16 && c == 16 && d == 32 && B.bytes == 64, "regions at %zu %zu %zu %zu of %zu bytes", a, b, c, d, B.bytes);
    alignas(16) unsigned char block[64] = {};
    CHECK((void *)BlockLayout::at<uint32_t>(block, d) == (void *)(block + 32), "a region's address");
    return true;
}

int main() {
    if (!check_prefix() || !check_lookup() || !check_layout()) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
