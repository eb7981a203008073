// analysis_plan_test.cpp — the analysis geometry (flo_amd/csrc/analysis_plan.cpp) on the host. Without arguments it runs
// its own cases - the thresholds every scan changes its path at, and the bounds the kernels rely on when they index their
// scratch - prints "ok <checks>" and returns 0, or names the first case that fails. With "dump" it reads lines
// "n sample_rate channels peaks_per_second" from stdin and prints the geometry, the work lists' items and their
// workgroups, one line per clip (tests/test_analysis_model_cpu.py compares tests/analysis_model.py with that).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../flo_amd/csrc/analysis_plan.hpp"

using namespace flo;

static long checks = 0;
#define CHECK(c, ...)                             \
    do {                                          \
        checks++;                                 \
        if (!(c)) {                               \
            printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
            printf(__VA_ARGS__);                  \
            printf("\n");                         \
            return 1;                             \
        }                                         \
    } while (0)

static AnalysisPlan plan(uint64_t n, uint32_t sr, unsigned ch, uint32_t pps, std::vector<uint64_t> *bl = nullptr) {
    AnalysisPlan P;
    analysis_plan(P, (size_t)n, sr, (uint8_t)ch, pps, bl);
    return P;
}

static void dump(const AnalysisPlan &P) {
    printf("%u %u %u %u %u %u %u %u %u %u %u %u %llu %llu %llu %llu %llu %u %u %u", P.n_peaks, P.hop, P.n_blocks, P.seg_frames, P.warm_frames,
           P.n_seg, P.fast, P.kseg_frames, P.n_kseg, P.kq, P.sq_exact, P.n_sq_seg, P.n_sq_chunks, P.n_chunks, P.points[0], P.points[1],
           P.points[2], P.point_ok[0], P.point_ok[1], P.point_ok[2]);
    unsigned long long it[kAnlCount];
    an_batch_items(P, it);
    printf(" |");
    for (int k = 0; k < kAnlCount; k++) printf(" %llu", it[k]);
    printf(" |");
    for (int k = 0; k < kAnlCount; k++) printf(" %llu", (it[k] + an_batch_per_wg(k) - 1) / an_batch_per_wg(k));
    printf(" | %a", P.samples_per_peak);
    for (int i = 0; i < 5; i++) printf(" %a", P.shelf[i]);
    for (int i = 0; i < 5; i++) printf(" %a", P.hp[i]);
    for (int i = 0; i < 16; i++) printf(" %a", P.kpow[i]);
    for (int i = 0; i < 49; i++) printf(" %a", P.tp_coef[i]);
    printf("\n");
}

static int own_cases() {
    // which K-weighting path: one walk up to 65 536 frames, two passes beyond for up to 64 channels, warm-up segments above
    CHECK(!plan(65536, 8000, 1, 50).fast && plan(65537, 8000, 1, 50).fast, "65536 / 65537 frames");
    CHECK(plan(65537ull * 64, 8000, 64, 50).fast && !plan(65537ull * 65, 8000, 65, 50).fast, "64 / 65 channels");
    CHECK(plan(65537ull * 65, 8000, 65, 50).n_seg == 2 && plan(65536ull * 65, 8000, 65, 50).n_seg == 1, "warm-up segments");
    CHECK(plan(2ull * 65536 + 1, 8000, 2, 50).n_seg == 2, "a trailing partial frame counts for the segments");
    CHECK(plan(700000, 96000, 1, 50).seg_frames == 76800 && plan(700000, 192000, 1, 50).seg_frames == 153600, "seg_frames = 8 hop");
    CHECK(plan(700000, 44100, 1, 50).warm_frames == 11025 && plan(700000, 8000, 1, 50).warm_frames == 8192, "warm_frames");
    // the short segments' length: 256 up to 2^19 frames, 512 up to 2^21, 1024 up to 2^23, 2048 beyond
    const uint64_t edge[3] = {524288, 2097152, 8388608};
    for (int i = 0; i < 3; i++) {
        CHECK(plan(edge[i], 4000, 1, 50).kseg_frames == (256u << i), "kseg at %" PRIu64, edge[i]);
        CHECK(plan(edge[i] + 1, 4000, 1, 50).kseg_frames == (512u << i), "kseg behind %" PRIu64, edge[i]);
    }
    CHECK(plan(8388609, 4000, 1, 50).kq == 7 && plan(8388609, 4000, 1, 50).hop == 400, "kq at 4 kHz");
    // sum of squares, hash chunks, FFT points
    CHECK(!plan(65536, 44100, 2, 50).sq_exact && plan(65537, 44100, 2, 50).sq_exact, "sum-of-squares chain beyond 65536 samples");
    CHECK(plan(65537, 44100, 2, 50).n_sq_chunks == 65 && plan(65537, 44100, 2, 50).n_sq_seg == 1, "chunks of the chain");
    CHECK(plan(253, 16000, 1, 50).n_chunks == 1 && plan(254, 16000, 1, 50).n_chunks == 2, "9 + 4 n bytes in 1 KiB chunks");
    CHECK(!plan(341, 16000, 1, 50).point_ok[0] && plan(342, 16000, 1, 50).point_ok[0], "first FFT point from 342 frames");
    CHECK(!plan(512, 16000, 1, 50).point_ok[1] && plan(513, 16000, 1, 50).point_ok[1], "second FFT point from 513 frames");
    CHECK(!plan(1024, 16000, 1, 50).point_ok[2] && plan(1025, 16000, 1, 50).point_ok[2] && !plan(1024, 16000, 1, 50).point_ok[2], "third FFT point from 1025 frames");
    // peak windows: more windows a second than samples leaves windows empty but counted; none starts behind the clip
    CHECK(plan(1000, 44100, 1, 100000).n_peaks == 2268, "pps > rate: %u", plan(1000, 44100, 1, 100000).n_peaks);
    CHECK(plan(0, 44100, 2, 50).n_peaks == 0 && plan(1, 44100, 2, 50).n_peaks == 1, "empty and one-sample clips");
    // bounds the kernels index by, over a sweep
    const uint32_t rates[] = {1, 4, 5, 2000, 3400, 4000, 8000, 11025, 22050, 44100, 48000, 96000, 192000};
    const unsigned chans[] = {1, 2, 3, 6, 64, 65, 255};
    const uint64_t lens[] = {1, 255, 256, 65535, 65536, 65537, 76799, 76800, 76801, 140000, 153601, 524287, 524288, 524289, 2097153, 8388609};
    for (uint32_t sr : rates)
        for (unsigned ch : chans)
            for (uint64_t fr : lens)
                for (unsigned extra = 0; extra < 2; extra++) {
                    if (fr * ch > 40000000ull || fr * 50 / sr > 5000000ull) continue;   // (keeps the run short: peak windows are counted one by one)
                    const uint64_t n = fr * ch + (extra && ch > 1 ? ch - 1 : 0);
                    std::vector<uint64_t> bl;
                    const AnalysisPlan P = plan(n, sr, ch, 50, &bl);
                    const uint64_t frames = n / ch;
                    CHECK(bl.size() == P.n_blocks, "block lengths");
                    if (P.hop) {
                        const uint64_t want = frames <= 4ull * P.hop ? (frames ? 1 : 0) : (frames - 4ull * P.hop + P.hop - 1) / P.hop + 1;
                        CHECK(P.n_blocks == want, "n_blocks %u want %" PRIu64 " (%" PRIu64 " frames, hop %u)", P.n_blocks, want, frames, P.hop);
                        CHECK(8ull * P.hop <= P.seg_frames, "a block spans at most two segments");
                    } else {
                        CHECK(P.n_blocks == 0 && !P.fast, "no hop, no blocks");
                    }
                    CHECK((uint64_t)P.n_kseg * P.kseg_frames >= frames && (P.n_kseg == 0 || (uint64_t)(P.n_kseg - 1) * P.kseg_frames < frames), "n_kseg");
                    CHECK((uint64_t)P.n_seg * P.seg_frames >= (n + ch - 1) / ch, "n_seg");
                    if (P.fast) {
                        // the quantum slots a segment may write: one per edge inside its kseg_frames (padded lanes included), and one
                        unsigned worst = 0;
                        for (unsigned off = 0; off < P.hop && off < 4096; off++) {
                            unsigned e = 0;
                            for (uint64_t x = P.hop - off; x < P.kseg_frames; x += P.hop) e++;
                            worst = e > worst ? e : worst;
                        }
                        CHECK(worst + 1 <= P.kq, "kq %u holds %u slots", P.kq, worst + 1);
                        CHECK(P.kseg_frames % 8 == 0 && frames > 65536 && ch <= 64, "fast path's conditions");
                    }
                    CHECK(P.sq_exact == (n > 65536 ? 1u : 0u) && P.n_sq_chunks == (n + 1023) / 1024, "sum-of-squares geometry");
                    CHECK(P.n_chunks * 1024 >= 9 + 4 * n && (P.n_chunks - 1) * 1024 < 9 + 4 * n, "hash chunks");
                    for (int i = 0; i < 3; i++) CHECK(!P.point_ok[i] || P.points[i] + 256 < frames, "an FFT window inside the whole frames");
                    CHECK(P.n_peaks >= 1 && (uint64_t)((double)(P.n_peaks - 1) * P.samples_per_peak) * ch < n, "the last peak window starts inside");
                    // a clip planned after another of its rate gets the same plan as alone
                    AnalysisPlan Q, like = plan(70000ull * ch, sr, ch, 50);
                    analysis_plan(Q, (size_t)n, sr, (uint8_t)ch, 50, nullptr, false, &like);
                    CHECK(!memcmp(Q.shelf, P.shelf, sizeof P.shelf) && !memcmp(Q.hp, P.hp, sizeof P.hp) && !memcmp(Q.tp_coef, P.tp_coef, sizeof P.tp_coef) &&
                              !memcmp(Q.kpow, P.kpow, sizeof P.kpow) && Q.hop == P.hop && Q.kq == P.kq && Q.n_blocks == P.n_blocks,
                          "`like` changes nothing (%u Hz, %u ch, %" PRIu64 ")", sr, ch, n);
                    unsigned long long it[kAnlCount];
                    an_batch_items(P, it);
                    CHECK((it[kAnlLoud] != 0) != (it[kAnlKw] != 0) && (it[kAnlSumsq] != 0) != (it[kAnlSqChunk] != 0), "one path per scan");
                }
    printf("ok %ld\n", checks);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "dump")) {
        unsigned long long n;
        unsigned sr, ch, pps;
        while (scanf("%llu %u %u %u", &n, &sr, &ch, &pps) == 4) dump(plan(n, sr, ch, pps));
        return 0;
    }
    return own_cases();
}
