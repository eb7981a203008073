// The role map of lossy_chain2q_kernel (flo_amd/csrc/chain2q_roles.hpp), for every workgroup size g = 1 .. 6:
//  - the 2 g waves map one to one onto g slots x {transform, packer};
//  - the two waves of a slot sit on different SIMDs (waves w, w + 4, w + 8 share one);
//  - the busiest SIMD's instruction load is no higher than under the first rule (waves 0 .. g-1 transform, g .. 2g-1
//    pack, slot = w % g), and is the minimum over ALL assignments of g transform and g packer roles to the 2 g waves;
//  - g = 6 (the many-round launches) is the first rule unchanged; every g at which the first rule is a minimum keeps its
//    roles, and its slots too except at g = 4, where the first rule puts both waves of a slot on one SIMD;
//  - no SIMD holds three waves of one role (measured: of three packers at one priority the youngest starves);
//  - the rank helpers agree with a direct count.
#include <stdio.h>

#include "../../flo_amd/csrc/chain2q_roles.hpp"

using namespace flo;

static int fails = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            fails++;                           \
            fprintf(stderr, "FAIL %s: ", #c);  \
            fprintf(stderr, __VA_ARGS__);      \
            fprintf(stderr, "\n");             \
        }                                      \
    } while (0)

// largest per-SIMD load when the waves in `packers` (a bit per wave) pack and the others transform
static int max_load(int g, unsigned packers) {
    int load[kChain2qSimds] = {0, 0, 0, 0}, m = 0;
    for (int w = 0; w < 2 * g; w++) load[w % kChain2qSimds] += (packers >> w & 1u) ? kChain2qWeightP : kChain2qWeightT;
    for (int s = 0; s < kChain2qSimds; s++) m = load[s] > m ? load[s] : m;
    return m;
}

int main() {
    static_assert(chain2q_role(5, 0).slot == 0 && !chain2q_role(5, 0).packer, "usable in constant expressions");
    static_assert(kChain2qWeightT > kChain2qWeightP, "the worked cases assume the transform wave is the heavier one");
    for (int g = 1; g <= kChain2qMaxSlots; g++) {
        int seen[kChain2qMaxSlots][2] = {};
        int wave_of[kChain2qMaxSlots][2] = {};
        unsigned packers = 0, packers_old = 0;
        for (int w = 0; w < 2 * g; w++) {
            const Chain2qRole r = chain2q_role(g, w);
            CHECK(r.slot >= 0 && r.slot < g, "g=%d wave %d: slot %d", g, w, r.slot);
            if (r.slot < 0 || r.slot >= g) continue;
            seen[r.slot][r.packer]++;
            wave_of[r.slot][r.packer] = w;
            if (r.packer) packers |= 1u << w;
            if (w >= g) packers_old |= 1u << w;
        }
        for (int s = 0; s < g; s++) {
            CHECK(seen[s][0] == 1 && seen[s][1] == 1, "g=%d slot %d: %d transform, %d packer waves", g, s, seen[s][0], seen[s][1]);
            CHECK(wave_of[s][0] % kChain2qSimds != wave_of[s][1] % kChain2qSimds, "g=%d slot %d: waves %d and %d share a SIMD", g, s,
                  wave_of[s][0], wave_of[s][1]);
        }
        const int mine = max_load(g, packers), old = max_load(g, packers_old);
        CHECK(mine <= old, "g=%d: max SIMD load %d above the first rule's %d", g, mine, old);
        // the minimum over every choice of g packers among 2 g waves (a slot pairing on different SIMDs exists for the
        // map under test; an unpairable choice can only lower the bound, so the check is not weakened by counting it)
        int best = old;
        for (unsigned m = 0; m < (1u << (2 * g)); m++) {
            if (__builtin_popcount(m) != g) continue;
            const int l = max_load(g, m);
            best = l < best ? l : best;
        }
        CHECK(mine == best, "g=%d: max SIMD load %d, the minimum is %d", g, mine, best);
        // where the first rule's roles are a minimum they stay; at g = 6 its slots stay too (at g = 4 they cannot: its
        // waves s and s + 4 share a SIMD)
        if (old == best)
            for (int w = 0; w < 2 * g; w++) {
                const Chain2qRole r = chain2q_role(g, w);
                CHECK(r.packer == (w >= g), "g=%d wave %d: role differs from the first rule's, which is a minimum here", g, w);
                if (g != 4) CHECK(r.slot == w % g, "g=%d wave %d: slot %d differs from the first rule's", g, w, r.slot);
            }
        CHECK(g != kChain2qMaxSlots || old == best, "g=%d: the first rule must be a minimum at the largest workgroup", g);
        for (int w = 0; w < 2 * g; w++) {
            int rank = 0, on = 0;
            for (int v = 0; v < 2 * g; v++)
                if (v % kChain2qSimds == w % kChain2qSimds && chain2q_role(g, v).packer == chain2q_role(g, w).packer) {
                    on++;
                    rank += v < w;
                }
            CHECK(chain2q_rank_on_simd(g, w) == rank, "g=%d wave %d: rank %d, counted %d", g, w, chain2q_rank_on_simd(g, w), rank);
            CHECK(chain2q_peers_on_simd(g, w) == on, "g=%d wave %d: %d waves of its role on its SIMD, counted %d", g, w,
                  chain2q_peers_on_simd(g, w), on);
            CHECK(on <= 2, "g=%d wave %d: %d waves of one role on its SIMD (of three the youngest starves)", g, w, on);
        }
        printf("g=%d max SIMD load %d (first rule %d, minimum %d)\n", g, mine, old, best);
    }
    // the worked case of g = 5
    CHECK(max_load(5, 0x3E0u) == 2 * kChain2qWeightT + kChain2qWeightP, "first rule at g=5");
    {
        unsigned p5 = 0;
        for (int w = 0; w < 10; w++) p5 |= chain2q_role(5, w).packer ? 1u << w : 0u;
        CHECK(max_load(5, p5) == kChain2qWeightT + 2 * kChain2qWeightP, "g=5: %d", max_load(5, p5));
    }
    if (fails) {
        fprintf(stderr, "%d check(s) failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
