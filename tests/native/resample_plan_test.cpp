// resample_plan_test.cpp — the host side of sample-rate conversion (flo_amd/csrc/resample_plan.cpp and the inline index
// arithmetic of resample_plan.hpp that the kernel shares): where every output lies, how many a clip has, that the tiles of a
// batch make every output exactly once and nothing else, and that what a tile stages fits the LDS the kernel may take.
// Prints "ok <checks>" and returns 0, or names the first case that fails.
// With the argument "dump" it reads lines "in_rate out_rate n_in ..." from stdin and prints, per line, the plan's fields and
// "n_out:tiles" of every clip length, or "rejected: <message>" (tests/test_resample_model_cpu.py compares them with
// tests/resample_model.py). With the argument "check" it reads rate pairs from stdin and runs the geometry, count and table
// checks below on each (every pair must be a supported one), then prints "ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../flo_amd/csrc/clip_tiles.hpp"
#include "../../flo_amd/csrc/resample_plan.hpp"

using namespace flo;
typedef unsigned __int128 u128;

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

// (i, p) of output j against a 128-bit evaluation
static bool check_pos() {
    const uint32_t Ls[] = {1, 2, 3, 80, 147, 160, 441, 1023, 1024};
    const uint32_t Ms[] = {1, 2, 80, 147, 160, 320, 441, 4095, 384000};
    const uint64_t js[] = {0, 1, 2, 146, 147, 148, 1000003, (1ull << 31) - 1, 1ull << 31, (1ull << 32) + 5, (1ull << 40) - 1, 1ull << 40};
    for (uint32_t L : Ls)
        for (uint32_t M : Ms)
            for (uint64_t j : js) {
                uint64_t i;
                uint32_t p;
                resample_pos(j, L, M, i, p);
                const u128 t = (u128)j * M;
                CHECK((u128)i == t / L && (u128)p == t % L, "resample_pos(j=%llu, L=%u, M=%u) = (%llu, %u)", (unsigned long long)j, L, M,
                      (unsigned long long)i, p);
            }
    return true;
}

static bool check_out_frames(const ResamplePlan &P) {
    const uint64_t M = P.M;
    const uint64_t ns[] = {0, 1, M - 1, M, M + 1, 1ull << 40};
    for (uint64_t n : ns) {
        uint64_t got = 0;
        const u128 want = ((u128)n * P.L + M - 1) / M;
        CHECK(resample_out_frames(P, n, got) && (u128)got == want, "%u -> %u: out_frames(%llu) = %llu", P.in_rate, P.out_rate,
              (unsigned long long)n, (unsigned long long)got);
    }
    uint64_t z = 1;
    CHECK(resample_out_frames(P, 0, z) && z == 0, "0 frames give 0");
    return true;
}

// The plan's own invariants, and a batch of clips through the kernel's mapping: tile -> unit -> lane -> output.
static bool check_geometry(const ResamplePlan &P) {
    const uint32_t L = P.L, M = P.M, T = P.taps;
    CHECK(T % 2 == 0 && T >= 64 && T <= kResampleMaxTaps && L <= kResampleMaxPhases, "%u -> %u: taps %u, L %u", P.in_rate, P.out_rate, T, L);
    CHECK(P.tile_outputs == P.slots * L && P.slots >= 1, "tile_outputs");
    CHECK(P.lanes_per_phase == (P.slots < 64 ? P.slots : 64) && P.phases_per_wave == 64 / P.lanes_per_phase && P.phases_per_wave >= 1, "lanes");
    CHECK(P.chunks == (P.slots + 63) / 64 && (P.chunks == 1 || P.slots % 64 == 0), "chunks");
    CHECK(P.block == (P.phases_per_wave == 1 ? kResampleBlock : 1u), "block");
    CHECK(P.units == P.chunks * ((L + P.phases_per_wave * P.block - 1) / (P.phases_per_wave * P.block)), "units");
    CHECK(P.span == resample_span(L, M, T, P.slots) && P.lds_elems == resample_lds_index(P.span - 1, P.shift) + 1, "span");
    // the LDS budget the kernel is compiled for, at every channel count; two workgroups per CU
    for (uint32_t ch = 1; ch <= 8; ch++) {
        const uint32_t bytes = resample_lds_bytes(P, ch);
        CHECK(bytes == P.lds_elems * 4 * (ch >= 2 ? 2 : 1) && bytes <= kResampleLdsBytes, "%u -> %u: %u channels take %u bytes of LDS", P.in_rate,
              P.out_rate, ch, bytes);
    }
    CHECK(2 * kResampleLdsBytes <= 160 * 1024, "two workgroups per CU");
    // the lanes' stride in LDS is odd: 32 consecutive slots fall in 32 banks
    CHECK(((M + (M >> P.shift)) & 1u) == 1u, "%u -> %u: stride %u", P.in_rate, P.out_rate, M + (M >> P.shift));
    CHECK(P.shift == 31 ? (M & 1u) == 1u : (M % (1u << P.shift) == 0 && ((M >> P.shift) & 1u) == 1u), "shift");

    // clips: empty, one frame, a few frames, one tile exactly, around a tile, several tiles
    const uint64_t tile = P.tile_outputs;
    const std::vector<uint64_t> n_out = {0, 1, 0, 2, T / 2, tile - 1, tile, tile + 1, 2 * tile + 17, 0};
    std::vector<uint32_t> pre;
    CHECK(clip_tiles(n_out.data(), n_out.size(), P.tile_outputs, pre) && pre.size() == n_out.size() + 1 && pre[0] == 0, "tiles");
    for (size_t c = 0; c < n_out.size(); c++) CHECK(pre[c + 1] - pre[c] == (n_out[c] + tile - 1) / tile, "clip %zu: tiles", c);
    std::vector<std::vector<uint8_t>> made(n_out.size());
    for (size_t c = 0; c < n_out.size(); c++) made[c].assign(n_out[c], 0);
    for (uint32_t b = 0; b < pre.back(); b++) {
        // the kernel's search: the last clip with pre[lo] <= b
        uint32_t lo = 0, hi = (uint32_t)n_out.size();
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pre[mid] <= b) lo = mid;
            else hi = mid;
        }
        CHECK(pre[lo] <= b && b < pre[lo + 1], "block %u lands in clip %u", b, lo);
        const uint32_t t = b - pre[lo];
        const uint64_t j0 = (uint64_t)t * tile;
        uint64_t i0;
        uint32_t p0;
        resample_pos(j0, L, M, i0, p0);
        CHECK(p0 == 0, "a tile starts at phase 0");
        const int64_t start = (int64_t)i0 - (int64_t)(T / 2 - 1);
        for (uint32_t unit = 0; unit < P.units; unit++) {
            uint32_t r_first = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const ResampleLane ln = resample_lane(unit, lane, L, P.slots, P.lanes_per_phase, P.phases_per_wave, P.chunks, P.block);
                if (lane == 0) {
                    r_first = ln.r;
                    CHECK(ln.r < L, "lane 0 of unit %u has a phase", unit);
                }
                if (!ln.active) continue;
                if (P.phases_per_wave == 1) CHECK(ln.r == r_first, "one phase per wave: unit %u lane %u", unit, lane);
                CHECK(ln.q < P.slots && ln.r < L, "unit %u lane %u: slot %u phase %u", unit, lane, ln.q, ln.r);
                uint32_t e_prev = 0;
                for (uint32_t b2 = 0; b2 < P.block && ln.r + b2 < L; b2++) {
                    const uint32_t r = ln.r + b2;
                    uint32_t e0, p;
                    resample_phase(r, L, M, e0, p);
                    // the windows of a block start in order, less than a window apart: the kernel's prologue and epilogue
                    CHECK(b2 == 0 || (e0 >= e_prev && e0 - e_prev < T), "block of phase %u: windows", ln.r);
                    if (b2 == 0) e_prev = e0;
                    const uint64_t j = j0 + (uint64_t)ln.q * L + r;
                    uint64_t i;
                    uint32_t pj;
                    resample_pos(j, L, M, i, pj);
                    // the row it uses and the frames it reads are the definition's
                    CHECK(pj == p, "output %llu: row %u, the definition says %u", (unsigned long long)j, p, pj);
                    const uint64_t f0 = (uint64_t)ln.q * M + e0;
                    CHECK(start + (int64_t)f0 == (int64_t)i - (int64_t)(T / 2) + 1, "output %llu: first tap", (unsigned long long)j);
                    CHECK(f0 + T <= P.span, "output %llu reads past the staged span", (unsigned long long)j);
                    const uint32_t o_last = e0 + T - 1, a_last = ln.q * (M + (M >> P.shift)) + o_last + (o_last >> P.shift);
                    CHECK(a_last == resample_lds_index((uint32_t)f0 + T - 1, P.shift) && a_last < P.lds_elems, "output %llu: LDS index",
                          (unsigned long long)j);
                    if (j < n_out[lo]) {
                        CHECK(made[lo][j] == 0, "clip %u output %llu is made twice", lo, (unsigned long long)j);
                        made[lo][j] = 1;
                    }
                }
            }
        }
    }
    for (size_t c = 0; c < n_out.size(); c++)
        for (uint64_t j = 0; j < n_out[c]; j++) CHECK(made[c][j] == 1, "clip %zu output %llu is not made", c, (unsigned long long)j);
    // the LDS image is one to one
    std::vector<uint8_t> used(P.lds_elems, 0);
    for (uint32_t f = 0; f < P.span; f++) {
        const uint32_t a = resample_lds_index(f, P.shift);
        CHECK(a < P.lds_elems && !used[a], "staged frame %u", f);
        used[a] = 1;
    }
    return true;
}

static bool check_table(const ResamplePlan &P) {
    const std::vector<float> h = resample_table(P);
    CHECK(h.size() == (size_t)P.L * P.taps, "table size");
    for (uint32_t p = 0; p < P.L; p++) {
        double s = 0;
        for (uint32_t k = 0; k < P.taps; k++) s += h[(size_t)p * P.taps + k];
        CHECK(s > 1 - 1e-5 && s < 1 + 1e-5, "%u -> %u: row %u sums to %.9f", P.in_rate, P.out_rate, p, s);
    }
    return true;
}

// one line of stdin per rate pair: "in_rate out_rate n_in n_in ..."
static int dump() {
    char *line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, stdin) > 0) {
        char *s = line;
        const unsigned long long a = strtoull(s, &s, 10), b = strtoull(s, &s, 10);
        ResamplePlan P;
        std::string err;
        if (a > 0xFFFFFFFFull || b > 0xFFFFFFFFull || !resample_plan((uint32_t)a, (uint32_t)b, P, err)) {
            printf("rejected: %s\n", err.c_str());
            continue;
        }
        printf("%u %u %u %u %u %u %u %u %u %u %u %u %u |", P.L, P.M, P.taps, P.shift, P.slots, P.lanes_per_phase, P.phases_per_wave, P.chunks,
               P.block, P.units, P.span, P.lds_elems, P.tile_outputs);
        std::vector<uint64_t> n_out;
        for (;;) {
            char *end;
            const unsigned long long n_in = strtoull(s, &end, 10);
            if (end == s) break;
            s = end;
            uint64_t n = 0;
            if (!resample_out_frames(P, n_in, n)) return fprintf(stderr, "out_frames(%llu)\n", n_in), 1;
            n_out.push_back(n);
        }
        std::vector<uint32_t> pre;
        if (!clip_tiles(n_out.data(), n_out.size(), P.tile_outputs, pre)) return fprintf(stderr, "tiles\n"), 1;
        for (size_t i = 0; i < n_out.size(); i++) printf(" %llu:%u", (unsigned long long)n_out[i], pre[i + 1] - pre[i]);
        printf("\n");
    }
    free(line);
    return 0;
}

static int check_pairs() {
    unsigned a, b;
    while (scanf("%u %u", &a, &b) == 2) {
        ResamplePlan P;
        std::string err;
        if (!resample_plan(a, b, P, err)) return fprintf(stderr, "%u -> %u: %s\n", a, b, err.c_str()), 1;
        if (!check_out_frames(P) || !check_geometry(P) || !check_table(P)) return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "dump")) return dump();
    if (argc > 1 && !strcmp(argv[1], "check")) return check_pairs();
    if (!check_pos()) return 1;
    const uint32_t pairs[][2] = {{48000, 44100}, {44100, 48000}, {96000, 44100}, {8000, 44100}, {44100, 8000}, {44100, 22050},
                                 {22050, 44100}, {48000, 48000}, {44100, 44101}, {384000, 8000}};
    for (auto &pr : pairs) {
        ResamplePlan P;
        std::string err;
        const bool ok = resample_plan(pr[0], pr[1], P, err);
        const bool rejected = (pr[0] == 44100 && pr[1] == 44101) || (pr[0] == 384000 && pr[1] == 8000);
        g_checks++;
        if (ok == rejected) {
            fprintf(stderr, "%u -> %u: %s\n", pr[0], pr[1], ok ? "accepted" : err.c_str());
            return 1;
        }
        if (rejected) {
            g_checks++;
            const char *name = pr[1] == 44101 ? "L" : "taps";
            if (err.find(name) == std::string::npos) {
                fprintf(stderr, "%u -> %u: the message does not name %s: %s\n", pr[0], pr[1], name, err.c_str());
                return 1;
            }
            continue;
        }
        if (!check_out_frames(P) || !check_geometry(P) || !check_table(P)) return 1;
    }
    // the table of the issue: L and taps of the common conversions
    const uint32_t want[][4] = {{48000, 44100, 147, 70}, {44100, 48000, 160, 64}, {96000, 44100, 147, 140}, {8000, 44100, 441, 64},
                                {44100, 8000, 80, 354}, {44100, 22050, 1, 128}};
    for (auto &w : want) {
        ResamplePlan P;
        std::string err;
        g_checks++;
        if (!resample_plan(w[0], w[1], P, err) || P.L != w[2] || P.taps != w[3]) {
            fprintf(stderr, "%u -> %u: L %u taps %u\n", w[0], w[1], P.L, P.taps);
            return 1;
        }
    }
    // the limits name what they refuse
    {
        ResamplePlan P;
        std::string err;
        g_checks += 3;
        if (resample_plan(0, 44100, P, err) || err.find("in_rate") == std::string::npos) return fprintf(stderr, "in_rate 0: %s\n", err.c_str()), 1;
        if (resample_plan(44100, 384001, P, err) || err.find("out_rate") == std::string::npos) return fprintf(stderr, "out_rate: %s\n", err.c_str()), 1;
        // L = 1001, M = 4100: 264 taps, a table of 1 057 056 bytes
        if (resample_plan(369000, 90090, P, err) || err.find("table") == std::string::npos) return fprintf(stderr, "369000 -> 90090: %s\n", err.c_str()), 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
