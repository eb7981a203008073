// chain2q_roles.hpp — which wave of a lossy_chain2q_kernel workgroup serves which clip slot, and in which role.
// Shared by the kernel, its launcher and tests/native/chain2q_roles_test.cpp (plain C++, no HIP needed).
//
// A workgroup of g clip slots has 2 g waves; waves w, w + 4, w + 8 share a SIMD (the hardware deals a workgroup's waves
// round-robin over the four SIMDs; which SIMD wave 0 gets differs from CU to CU). Every slot needs one transform wave
// (T) and one packer wave (P) on different SIMDs (they run concurrently and wait for each other), and a launch of a
// single round lasts as long as its slowest slot, so the map keeps the busiest SIMD's instruction load per frame round
// as low as it can be. The first rule of this kernel - waves 0 .. g-1 transform, g .. 2g-1 pack, slot = w % g - is such
// a minimum for every g but 5, where it loads the SIMDs (T,T,P) (T,P,P) (T,P) (T,P) and the slot whose transform wave
// is the younger one of (T,T,P) ends 18 % of the launch behind the median slot. The map below loads them
// (T,P,P) (T,P,P) (T,T) (T,P): no transform wave shares a SIMD with both another transform wave and a packer. Among
// the maps of minimal load it is the one measured fastest: (T,P,P) (P,P,P) (T,T) (T,T) has the same maximum and was
// 3 % slower than the first rule - of three packers on one SIMD the youngest starves. Within the map,
// a slot pairs a wave that is held up on its SIMD (a transform wave under two packers, the younger of two packers)
// with one that is not. At g = 4 the first rule's roles stay but its slots do not: waves s and s + 4 share a SIMD, so
// the packers serve the next slot over.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLO_ROLES_HD __host__ __device__
#else
#define FLO_ROLES_HD
#endif

namespace flo {

constexpr int kChain2qMaxSlots = 6;   // FLO_C2X_THREADS / 128
constexpr int kChain2qSimds = 4;
// vector + scalar + LDS instructions per stereo frame of one wave of either role (a SIMD with T,T,P issues
// 2840 per frame round, one with T,P,P 2720)
constexpr int kChain2qWeightT = 987;
constexpr int kChain2qWeightP = 867;

struct Chain2qRole {
    int slot;      // clip slot of the workgroup, 0 .. g-1
    bool packer;   // false: transform wave
};

// the first rule, as a word of one nibble per wave: slot | packer << 3
constexpr uint64_t chain2q_rule_word(int g) {
    uint64_t m = 0;
    for (int w = 0; w < 2 * g; w++) m |= (uint64_t)((w % g) | (w >= g ? 8 : 0)) << (4 * w);
    return m;
}
// g = 4, waves 0 .. 7: T0 T1 T2 T3 | P1 P2 P3 P0 (the first rule's roles; its slots put both waves of a slot on one SIMD)
constexpr uint64_t kChain2qWord4 = 0x8BA93210ull;
// g = 5, waves 0 .. 9: T0 T1 T2 T3 | P1 P0 T4 P4 | P2 P3
constexpr uint64_t kChain2qWord5 = 0xBAC4893210ull;

FLO_ROLES_HD constexpr uint64_t chain2q_role_word(int g) {
    constexpr uint64_t w1 = chain2q_rule_word(1), w2 = chain2q_rule_word(2), w3 = chain2q_rule_word(3), w6 = chain2q_rule_word(6);
    constexpr uint64_t w4 = kChain2qWord4, w5 = kChain2qWord5;
    return g == 1 ? w1 : g == 2 ? w2 : g == 3 ? w3 : g == 4 ? w4 : g == 5 ? w5 : w6;
}
FLO_ROLES_HD constexpr Chain2qRole chain2q_role(int g, int wave) {
    const unsigned n = (unsigned)(chain2q_role_word(g) >> (4 * wave)) & 15u;
    return Chain2qRole{(int)(n & 7u), (n & 8u) != 0};
}
// among the waves of its own role on its SIMD, how many are older (have a lower wave index) than this one
FLO_ROLES_HD constexpr int chain2q_rank_on_simd(int g, int wave) {
    int r = 0;
    for (int w = wave % kChain2qSimds; w < wave; w += kChain2qSimds) r += chain2q_role(g, w).packer == chain2q_role(g, wave).packer ? 1 : 0;
    return r;
}
// waves of its own role on this wave's SIMD, itself among them
FLO_ROLES_HD constexpr int chain2q_peers_on_simd(int g, int wave) {
    int r = 0;
    for (int w = wave % kChain2qSimds; w < 2 * g; w += kChain2qSimds) r += chain2q_role(g, w).packer == chain2q_role(g, wave).packer ? 1 : 0;
    return r;
}

}  // namespace flo
