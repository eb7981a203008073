// Host test of the lossless decode's routing (flo_amd/csrc/ll_route.cpp): which kernels take a channel wrapper and what
// LlWrapperList makes of a call's wrappers. Built with g++ and the sanitizers by tests/test_lldec_model_cpu.py.
//   decode_plan_test        checks ll_route at each of its limits from both sides and the list's invariants over a
//                           pseudo-random sweep; prints "ok" and exits 0 when everything holds
//   decode_plan_test dump   reads lines "k shift len samples force n_coeffs c0 c1 ..." from stdin, routes each wrapper,
//                           pushes it and prints "serial other tiles"; a line "list" prints the list (tile0, others,
//                           scratch offsets, scratch, max_tiles) and clears it. tests/lldec_model.py must agree line for line.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

#include "../../flo_amd/csrc/ll_route.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            fprintf(stderr, "FAIL %s: ", #cond);           \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
        }                                                  \
    } while (0)

static LlChannelDev make(unsigned k, unsigned shift, uint32_t len, uint32_t samples, unsigned n_coeffs, const int32_t *co) {
    int32_t c[12] = {0};
    for (unsigned i = 0; i < n_coeffs && i < 12; i++) c[i] = co[i];
    LlChannelDev d = ll_channel(1000, len, (uint8_t)n_coeffs, (uint8_t)shift, (uint8_t)k, c);
    d.samples = samples;
    return d;
}

static void print_list(const LlWrapperList &w) {
    printf("list %zu tiles %u max_tiles %u scratch %" PRIu64 "\n tile0", w.chs.size(), w.tiles(), w.max_tiles, w.scratch);
    for (unsigned t : w.tile0) printf(" %u", t);
    printf("\n others");
    for (unsigned o : w.others) printf(" %u", o);
    printf("\n out_off");
    for (const LlChannelDev &d : w.chs) printf(" %llu", d.out_off);
    printf("\n serial");
    for (int s : w.serial) printf(" %d", s);
    printf("\n");
}

static int dump() {
    LlWrapperList w;
    w.clear();
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "list", 4)) {
            print_list(w);
            w.clear();
            continue;
        }
        std::istringstream in(line);
        unsigned k, shift, force, nco;
        uint32_t len, samples;
        if (!(in >> k >> shift >> len >> samples >> force >> nco) || nco > 12) return 2;
        int32_t co[12] = {0};
        for (unsigned i = 0; i < nco; i++)
            if (!(in >> co[i])) return 2;
        const LlChannelDev d = make(k, shift, len, samples, nco, co);
        const LlRoute r = ll_route(d, force != 0);
        w.push(d, r);
        printf("%u %u %u\n", (unsigned)r.serial, (unsigned)r.other, r.tiles);
    }
    return 0;
}

static void limits() {
    const int32_t two[2] = {900, -100};
    const uint32_t tile_bytes = (uint32_t)kRiceTileBits / 8u;
    // k
    CHECK(ll_route(make(14, 10, 300, 100, 2, two), false).serial == 0, "k = 14 is parallel");
    CHECK(ll_route(make(15, 10, 300, 100, 2, two), false).serial == 1, "k = 15 is serial");
    CHECK(ll_route(make(15, 0, 300, 100, 0, two), false).serial == 0, "raw bytes have no k");
    CHECK(ll_route(make(15, 129, 300, 100, 0, two), false).serial == 1, "a fixed predictor with k = 15 is serial");
    // sum of |taps|
    const int32_t under[2] = {(1 << 21) - 5, -4}, at[2] = {-(1 << 21) + 4, 4};
    CHECK(ll_route(make(5, 10, 300, 100, 2, under), false).serial == 0, "sum 2^21 - 1 is parallel");
    CHECK(ll_route(make(5, 10, 300, 100, 2, at), false).serial == 1, "sum 2^21 is serial");
    CHECK(ll_route(make(5, 10, 0, 100, 2, at), false).serial == 1 && ll_route(make(5, 10, 0, 100, 2, at), false).tiles == 0, "... without bytes too");
    // shift, taken modulo 64
    CHECK(ll_route(make(5, 20, 300, 100, 2, two), false).serial == 0, "shift 20");
    CHECK(ll_route(make(5, 21, 300, 100, 2, two), false).serial == 1, "shift 21");
    CHECK(ll_route(make(5, 84, 300, 100, 2, two), false).serial == 0, "shift 84 = 64 + 20");
    CHECK(ll_route(make(5, 85, 300, 100, 2, two), false).serial == 1, "shift 85");
    CHECK(ll_route(make(5, 128 + 21, 300, 100, 0, two), false).serial == 0, "a fixed predictor's order byte is no shift");
    // stream length
    const uint32_t cap = 16u * 1024u * (uint32_t)kRiceTileBits;
    CHECK(ll_route(make(5, 10, cap, 100, 2, two), false).serial == 0 && ll_route(make(5, 10, cap, 100, 2, two), false).tiles == cap / tile_bytes, "len = cap");
    CHECK(ll_route(make(5, 10, cap + 1, 100, 2, two), false).serial == 1 && ll_route(make(5, 10, cap + 1, 100, 2, two), false).tiles == 0, "len = cap + 1");
    CHECK(ll_route(make(5, 0, cap + 1, 100, 0, two), false).serial == 0, "raw bytes are no stream");
    // tiles
    for (uint32_t len : {1u, tile_bytes - 1, tile_bytes, tile_bytes + 1, 64 * tile_bytes, 64 * tile_bytes + 1})
        CHECK(ll_route(make(5, 10, len, 100, 2, two), false).tiles == (len + tile_bytes - 1) / tile_bytes, "tiles of %u bytes", len);
    // others
    CHECK(ll_route(make(5, 10, 300, 3, 2, two), false).other == 0, "samples = order + 1 takes the rows");
    CHECK(ll_route(make(5, 10, 300, 2, 2, two), false).other == 1, "samples = order does not");
    CHECK(ll_route(make(5, 10, 0, 100, 2, two), false).other == 1, "taps without bytes");
    CHECK(ll_route(make(5, 130, 300, 100, 0, two), false).other == 1, "fixed");
    CHECK(ll_route(make(5, 0, 300, 100, 0, two), false).other == 1 && ll_route(make(5, 0, 0, 100, 0, two), false).other == 1, "raw, silent");
    // forced
    const LlRoute f = ll_route(make(5, 10, 300, 100, 2, two), true);
    CHECK(f.serial == 1 && f.tiles == 0 && f.other == 0, "forced serial: %u %u %u", (unsigned)f.serial, f.tiles, (unsigned)f.other);
}

static void invariants() {
    uint64_t x = 88172645463325252ull;
    auto rnd = [&](uint32_t n) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return (uint32_t)(x % n);
    };
    LlWrapperList w;
    for (int round = 0; round < 200; round++) {
        w.clear();
        CHECK(w.chs.empty() && w.tile0.size() == 1 && w.tile0[0] == 0 && w.serial.empty() && w.others.empty() && w.frs.empty() && !w.scratch &&
                  !w.max_tiles && !w.max_samples,
              "clear()");
        const unsigned frames = 1 + rnd(12), nch = 1 + rnd(3);
        uint64_t want_scratch = 0, out_sf = 0;
        unsigned want_max = 0, want_samples = 0, want_tiles = 0, n_other = 0;
        for (unsigned f = 0; f < frames; f++) {
            const uint32_t samples = rnd(4) ? 1 + rnd(3000) : rnd(14);
            const uint64_t before = w.scratch;
            const size_t first = w.chs.size();
            w.add_frame(out_sf, samples, rnd(2) != 0, nch, false, [&](unsigned) {
                int32_t co[12];
                for (int32_t &c : co) c = (int32_t)rnd(1 << 20) - (1 << 19);
                const unsigned kind = rnd(6);
                const unsigned nco = kind < 3 ? 1 + rnd(12) : 0;
                const unsigned shift = kind < 3 ? rnd(90) : kind == 3 ? 128 + rnd(6) : 0;
                const uint32_t len = kind == 5 || !rnd(9) ? 0 : 1 + rnd(40000);
                return make(rnd(17), shift, len, 0, nco, co);
            });
            const LlFrameDev &fd = w.frs.back();
            CHECK(fd.first_channel == first && fd.n_channels == nch && fd.samples == samples && fd.out_off == out_sf, "frame %u", f);
            CHECK(fd.scratch_off[0] == before && (nch < 2 || fd.scratch_off[1] == before + samples), "frame %u scratch_off", f);
            out_sf += samples;
            if (samples > want_samples) want_samples = samples;
        }
        CHECK(w.chs.size() == (size_t)frames * nch && w.tile0.size() == w.chs.size() + 1 && w.serial.size() == w.chs.size(), "sizes");
        for (size_t i = 0; i < w.chs.size(); i++) {
            const LlRoute r = ll_route(w.chs[i], false);
            CHECK(w.tile0[i + 1] >= w.tile0[i] && w.tile0[i + 1] - w.tile0[i] == r.tiles, "tile0 at %zu", i);
            CHECK(w.serial[i] == r.serial, "serial at %zu", i);
            CHECK(w.chs[i].out_off == want_scratch, "out_off at %zu", i);
            CHECK(!(r.serial && r.tiles), "a serial wrapper has no tiles (%zu)", i);
            if (r.other) {
                CHECK(n_other < w.others.size() && w.others[n_other] == i, "others at %zu", i);
                n_other++;
            }
            want_scratch += w.chs[i].samples;
            want_tiles += r.tiles;
            if (r.tiles > want_max) want_max = r.tiles;
        }
        CHECK(n_other == w.others.size(), "others: %u of %zu", n_other, w.others.size());
        CHECK(w.scratch == want_scratch && w.max_tiles == want_max && w.tiles() == want_tiles && w.max_samples == want_samples, "totals");
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "dump")) return dump();
    limits();
    invariants();
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
