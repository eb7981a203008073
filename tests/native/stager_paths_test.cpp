// The three upload routes of flo_amd/csrc/stager.cpp - the runtime's pageable copy (upload_direct), the pinned ring
// (upload_ring) and the two-thread split of upload_direct (FLO_UPLOAD_THREADS=2) - on the CPU, against a stand-in for the
// runtime whose device runs late (tests/native/hipstub_streams: streams are FIFOs of deferred ops, pinned copies read
// their source when they RUN, pageable copies snapshot it at the call; late_runtime.cpp's head has the whole model).
// Built by tests/test_stager_paths_cpu.py with g++, once under AddressSanitizer and UBSan and once under ThreadSanitizer;
// stager.cpp is compiled unchanged, and what it needs from devpool.hpp and stream_delay.hpp is defined below.
//
// Every check runs under both scheduling policies (lazy: nothing runs until something synchronises on it; eager: an op
// runs as soon as it heads its stream with its dependencies met), each named as it is in "FAIL [name, policy]":
//
//   path            FLO_UPLOAD_PATH=ring / direct gives that path (stager_upload_choice, and by the kind of copies the
//                   runtime saw); with neither set the probe runs, names one of the two and reports two positive rates.
//   small limit     a total of exactly kSmallUpload stays on the pageable path and makes no ring; one byte more makes it.
//   table           every byte arrives once and only the bytes asked for: after the final synchronise each destination
//                   equals what its source held AT THE CALL - the sources are overwritten as soon as stager_upload
//                   returns, which is the contract of stager.hpp that no GPU test can see - every guard byte is intact
//                   and the runtime copied exactly the bytes asked for. Over one stager per path, so s->cur carries over.
//   slot reuse      40 MiB in one call behind a gate, and 24 MiB + 24 MiB in two calls on two gated streams: the ring has
//                   32 MiB, so a slot is filled again while its first copy is still queued. Protects the
//                   `hipEventSynchronize(s->ev[k])` at the top of upload_ring's loop. The gate is opened by another thread
//                   once the uploading thread is blocked behind it (or has returned, when the wait is missing).
//   shutdown        stager_destroy with ring copies queued behind a gate that another thread opens: protects the
//                   `hipEventSynchronize(s->ev[i])` of stager_destroy (freeing a slot that queued copies read is a
//                   violation in the model, and the destinations would receive poison).
//   split aux_go    (second run, FLO_UPLOAD_THREADS=2) `stream` gated behind a queued memset of the destinations: the
//                   helper thread's half must land behind that memset. Protects hipStreamWaitEvent(aux_stream, aux_go).
//   split aux_ev    synchronising `stream` alone delivers the helper's half; the second stream is never synchronised.
//                   Protects hipStreamWaitEvent(stream, aux_ev).
//   allocation      the 2nd, 3rd, 4th hipHostMalloc and the 2nd event creation of ensure_ring fail in turn: the upload
//                   returns non-zero with a message, a later large upload works or fails cleanly, stager_destroy frees
//                   what exists once; and the same through probe().
//   worker pool     200 consecutive stager_memcpy_many calls of 0, 1 and more jobs than workers, pieces of kPiece +- 1.
//
// With FLO_UPLOAD_THREADS=2 the program runs path, table (pageable path), the two split checks and allocation: the checks
// whose uploads reach upload_direct with 16 MiB and two segments or more. The ring and the worker pool never read the switch.
// At the end of each policy's pass nothing is queued, every block, event and stream the runtime handed out is back, and
// the model has counted no violation.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "devpool.hpp"
#include "stager.hpp"
#include "stream_delay.hpp"

// ---- what stager.cpp links against besides the runtime -----------------------------------------------------------------
namespace flo {
std::atomic<int> g_pool_fill{-1};
std::atomic<int> g_stream_delay{-1};
hipError_t stream_delay_enqueue(hipStream_t s, int) { return hipstub::nop_async(s); }
}  // namespace flo

namespace {
using flo::Stager;
using flo::UploadSeg;

// stager.cpp's constants (in its anonymous namespace); "small limit" and "worker pool" hold them against its behaviour
constexpr size_t MiB = (size_t)1 << 20;
constexpr size_t kSlotBytes = 8 * MiB, kSmallUpload = 8 * MiB, kPiece = 512 << 10;
constexpr int kSlots = 4;

int g_failures = 0;
const char *g_policy = "lazy";

void fail(const char *check, const char *what, unsigned long long a = 0, unsigned long long b = 0) {
    fprintf(stderr, "FAIL [%s, %s]: %s (%llu, %llu)\n", check, g_policy, what, a, b);
    g_failures++;
}

void fill_random(char *p, size_t bytes, uint64_t seed) {
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        memcpy(p + i, &x, 8);
    }
    for (; i < bytes; i++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        p[i] = (char)x;
    }
}

// host sources, what they held at the call, and guarded device destinations
struct Bufs {
    std::vector<std::vector<char>> src, expect;
    std::vector<void *> dst;
    size_t total = 0;

    Bufs(const std::vector<size_t> &lens, uint64_t seed) {
        for (size_t i = 0; i < lens.size(); i++) {
            src.emplace_back(lens[i] + 1);   // (one byte more: an empty segment still has an address)
            fill_random(src.back().data(), lens[i], seed * 1000 + i);
            expect.emplace_back(src.back().begin(), src.back().begin() + lens[i]);
            void *d = nullptr;
            if (hipMalloc(&d, lens[i]) != hipSuccess) abort();
            memset(d, 0xCC, lens[i]);
            dst.push_back(d);
            total += lens[i];
        }
    }
    std::vector<UploadSeg> segs() const {
        std::vector<UploadSeg> s;
        for (size_t i = 0; i < src.size(); i++) s.push_back({dst[i], src[i].data(), expect[i].size()});
        return s;
    }
    void scribble_sources() {   // the caller reuses its buffers as soon as the call returns
        for (auto &v : src) memset(v.data(), 0xEE, v.size());
    }
    bool verify(const char *check) const {
        bool ok = true;
        for (size_t i = 0; i < dst.size(); i++) {
            const size_t n = expect[i].size();
            if (n && memcmp(dst[i], expect[i].data(), n)) {
                size_t at = 0;
                while (((const char *)dst[i])[at] == expect[i][at]) at++;
                fprintf(stderr, "  segment %zu of %zu bytes: first difference at byte %zu: %02x, expected %02x\n", i, n, at,
                        (unsigned char)((const char *)dst[i])[at], (unsigned char)expect[i][at]);
                fail(check, "a destination differs from what its source held at the call", i, at);
                ok = false;
            }
            if (!hipstub::guards_intact(dst[i])) {
                fail(check, "guard bytes of a destination were overwritten", i, n);
                ok = false;
            }
        }
        return ok;
    }
    ~Bufs() {
        for (void *d : dst) hipFree(d);
    }
};

void use_path(const char *path) {
    if (path) setenv("FLO_UPLOAD_PATH", path, 1);
    else unsetenv("FLO_UPLOAD_PATH");
}
const char *name_of(const char *path) { return !strcmp(path, "ring") ? "pinned-ring" : "pageable-direct"; }

Stager *make_stager() {
    std::string err;
    Stager *s = flo::stager_create(err);
    if (!s) abort();
    return s;
}
hipStream_t make_stream() {
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) abort();
    return st;
}

// upload, overwrite the sources, synchronise, compare, and hold the runtime's byte count against the bytes asked for
bool upload_and_verify(const char *check, Stager *s, hipStream_t st, Bufs &b, bool count_bytes = true) {
    hipstub::reset_copy_counts();
    std::string err;
    if (flo::stager_upload(s, b.segs(), st, err) != 0) {
        fail(check, ("stager_upload failed: " + err).c_str());
        return false;
    }
    b.scribble_sources();
    if (hipStreamSynchronize(st) != hipSuccess) fail(check, "hipStreamSynchronize failed");
    bool ok = b.verify(check);
    const hipstub::Counts c = hipstub::counts();
    if (count_bytes && c.copied_bytes != b.total) {
        fail(check, "the runtime copied another number of bytes than the segments hold", c.copied_bytes, b.total);
        ok = false;
    }
    return ok;
}

// which path the runtime saw: pinned sources or pageable ones
void expect_copies(const char *check, const char *path, size_t total) {
    const hipstub::Counts c = hipstub::counts();
    const bool ring = !strcmp(path, "ring") && total > kSmallUpload;
    if (ring && (c.pageable_copies || !c.pinned_copies)) fail(check, "a large upload on the ring path was not copied from pinned memory", c.pinned_copies, c.pageable_copies);
    if (!ring && total && (c.pinned_copies || !c.pageable_copies)) fail(check, "an upload on the pageable path was copied from pinned memory", c.pinned_copies, c.pageable_copies);
}

// ---- path ---------------------------------------------------------------------------------------------------------------
void check_paths() {
    const char *check = "path";
    for (const char *path : {"ring", "direct"}) {
        use_path(path);
        Stager *s = make_stager();
        hipStream_t st = make_stream();
        if (strcmp(flo::stager_upload_choice(s, nullptr, nullptr), "not measured yet")) fail(check, "a choice is named before any large upload");
        Bufs b({kSmallUpload / 2, kSmallUpload / 2 + 1}, 1);
        upload_and_verify(check, s, st, b);
        expect_copies(check, path, b.total);
        if (strcmp(flo::stager_upload_choice(s, nullptr, nullptr), name_of(path))) fail(check, "stager_upload_choice does not name the path that was set");
        flo::stager_destroy(s);
        hipStreamDestroy(st);
    }
    use_path(nullptr);
    Stager *s = make_stager();
    hipStream_t st = make_stream();
    Bufs b({9 * MiB}, 2);
    upload_and_verify(check, s, st, b, false);   // (the probe's own copies are counted with it)
    double d = 0, r = 0;
    const char *choice = flo::stager_upload_choice(s, &d, &r);
    if (strcmp(choice, "pinned-ring") && strcmp(choice, "pageable-direct")) fail(check, "the probe named neither path");
    if (!(d > 0) || !(r > 0)) fail(check, "the probe did not report two positive rates");
    flo::stager_destroy(s);
    hipStreamDestroy(st);
}

// ---- small limit --------------------------------------------------------------------------------------------------------
void check_small_limit() {
    const char *check = "small limit";
    use_path("ring");
    Stager *s = make_stager();
    hipStream_t st = make_stream();
    const unsigned long long made = hipstub::counts().host_mallocs;
    {
        Bufs b({5 * MiB, 3 * MiB}, 3);   // exactly kSmallUpload
        upload_and_verify(check, s, st, b);
        expect_copies(check, "direct", b.total);
        if (strcmp(flo::stager_upload_choice(s, nullptr, nullptr), "not measured yet") || hipstub::counts().host_mallocs != made)
            fail(check, "a total of exactly kSmallUpload chose a path or made the ring");
    }
    {
        Bufs b({5 * MiB, 3 * MiB + 1}, 4);
        upload_and_verify(check, s, st, b);
        expect_copies(check, "ring", b.total);
        if (strcmp(flo::stager_upload_choice(s, nullptr, nullptr), "pinned-ring") || hipstub::counts().host_mallocs != made + kSlots)
            fail(check, "kSmallUpload + 1 did not take the ring", hipstub::counts().host_mallocs - made);
    }
    flo::stager_destroy(s);
    hipStreamDestroy(st);
}

// ---- table --------------------------------------------------------------------------------------------------------------
std::vector<std::vector<size_t>> table() {
    std::vector<std::vector<size_t>> t{{8 * MiB}, {8 * MiB + 4}, {8 * MiB - 4}};
    std::vector<size_t> many;   // as flo_decode and the corpus upload: lengths = 4 and = 60 (mod 64) and a few odd ones, 26 MiB in all
    for (size_t i = 0; i < 300; i++) {
        const size_t k = 1000 + (i * 37) % 700;
        many.push_back(i % 17 == 5 ? 64 * k + 33 : i % 23 == 7 ? 64 * k + 1 : i % 2 ? 64 * k + 60 : 64 * k + 4);
    }
    t.push_back(many);
    t.push_back({36 * MiB});                              // wraps the ring inside one call
    t.push_back({0, 5 * MiB + 1, 0, 4 * MiB + 3, 0});     // an empty segment first, in the middle and last
    t.push_back({5 * MiB, 3 * MiB});                      // exactly kSmallUpload
    t.push_back({5 * MiB, 3 * MiB + 1});
    return t;
}

bool g_split = false;   // FLO_UPLOAD_THREADS=2: the run that is about upload_direct

void check_table() {
    const char *check = "table";
    const auto lists = table();
    for (const char *path : {"ring", "direct"}) {
        if (g_split && !strcmp(path, "ring")) continue;
        use_path(path);
        Stager *s = make_stager();
        hipStream_t st = make_stream();
        for (size_t i = 0; i < lists.size(); i++) {
            Bufs b(lists[i], 10 + i);
            if (i == 3) {   // the list is what its comment says: upload_ring's cutting, replayed
                size_t fill = 0, cut = 0;
                for (size_t n : lists[i])
                    for (size_t left = n; left;) {
                        const size_t m = left < kSlotBytes - fill ? left : kSlotBytes - fill;
                        cut += m < left && m % 64 != left % 64;
                        fill = (fill + ((m + 63) & ~(size_t)63)) % kSlotBytes;
                        left -= m;
                    }
                if (b.total <= 2 * kSlotBytes || cut < 2) fail(check, "the list of many segments does not cross two slot boundaries inside segments", b.total, cut);
            }
            if (!upload_and_verify(check, s, st, b)) fprintf(stderr, "  (list %zu on the %s path)\n", i, path);
            expect_copies(check, path, b.total);
        }
        if (strcmp(flo::stager_upload_choice(s, nullptr, nullptr), name_of(path))) fail(check, "not the path that was set");
        flo::stager_destroy(s);
        hipStreamDestroy(st);
    }
}

// ---- slot reuse ---------------------------------------------------------------------------------------------------------
// opens `gates` once a host thread is blocked behind a closed gate, or once `returned` is set
std::thread opener(std::vector<int> gates, std::atomic<bool> &returned) {
    return std::thread([gates, &returned] {
        while (!returned.load() && !hipstub::gate_waiters()) std::this_thread::sleep_for(std::chrono::microseconds(200));
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
        for (int g : gates) hipstub::open_gate(g);
    });
}

void check_slot_reuse() {
    const char *check = "slot reuse";
    use_path("ring");
    {   // 40 MiB in one call: five slots' worth through four
        Stager *s = make_stager();
        hipStream_t st = make_stream();
        Bufs b({40 * MiB}, 20);
        std::atomic<bool> returned{false};
        std::thread t = opener({hipstub::gate(st)}, returned);
        std::string err;
        if (flo::stager_upload(s, b.segs(), st, err) != 0) fail(check, err.c_str());
        returned.store(true);
        b.scribble_sources();
        t.join();
        hipStreamSynchronize(st);
        b.verify(check);
        flo::stager_destroy(s);
        hipStreamDestroy(st);
    }
    {   // 24 MiB + 24 MiB in two calls on two streams, nothing synchronised between: s->cur carries over
        Stager *s = make_stager();
        hipStream_t st1 = make_stream(), st2 = make_stream();
        Bufs b1({24 * MiB}, 21), b2({11 * MiB + 4, 13 * MiB - 4}, 22);
        std::atomic<bool> returned{false};
        std::thread t = opener({hipstub::gate(st1), hipstub::gate(st2)}, returned);
        std::string err;
        if (flo::stager_upload(s, b1.segs(), st1, err) != 0) fail(check, err.c_str());
        b1.scribble_sources();
        if (flo::stager_upload(s, b2.segs(), st2, err) != 0) fail(check, err.c_str());
        returned.store(true);
        b2.scribble_sources();
        t.join();
        hipStreamSynchronize(st2);
        hipStreamSynchronize(st1);
        b1.verify(check);
        b2.verify(check);
        flo::stager_destroy(s);
        hipStreamDestroy(st1);
        hipStreamDestroy(st2);
    }
}

// ---- shutdown -----------------------------------------------------------------------------------------------------------
void check_shutdown() {
    const char *check = "shutdown";
    use_path("ring");
    Stager *s = make_stager();
    hipStream_t st = make_stream();
    Bufs b({24 * MiB}, 30);   // three slots: no reuse, so nothing has waited before stager_destroy
    std::atomic<bool> destroyed{false};
    std::thread t = opener({hipstub::gate(st)}, destroyed);
    const unsigned long long before = hipstub::counts().violations;
    std::string err;
    if (flo::stager_upload(s, b.segs(), st, err) != 0) fail(check, err.c_str());
    b.scribble_sources();
    flo::stager_destroy(s);
    destroyed.store(true);
    t.join();
    hipStreamSynchronize(st);
    b.verify(check);
    if (hipstub::counts().violations != before) fail(check, "the ring was freed while its copies were queued");
    hipStreamDestroy(st);
}

// ---- the split ----------------------------------------------------------------------------------------------------------
void check_split() {
    use_path("direct");
    const std::vector<size_t> lens{5 * MiB + 4, 5 * MiB, 5 * MiB + 60, 5 * MiB + 1};   // 20 MiB, four segments
    {
        const char *check = "split aux_go";
        Stager *s = make_stager();
        hipStream_t st = make_stream();
        const unsigned long long streams = hipstub::counts().streams_made;
        Bufs b(lens, 40);
        const int g = hipstub::gate(st);
        for (size_t i = 0; i < lens.size(); i++) hipstub::memset_async(b.dst[i], 0, lens[i], st);   // the batch's zero fill, still queued
        std::string err;
        if (flo::stager_upload(s, b.segs(), st, err) != 0) fail(check, err.c_str());
        if (hipstub::counts().streams_made != streams + 1) fail(check, "the split did not engage: no second stream was made");
        b.scribble_sources();
        hipstub::open_gate(g);
        hipStreamSynchronize(st);   // `stream` alone
        b.verify(check);
        hipstub::drain_all();
        flo::stager_destroy(s);
        hipStreamDestroy(st);
    }
    {
        const char *check = "split aux_ev";
        Stager *s = make_stager();
        hipStream_t st = make_stream();
        for (int round = 0; round < 2; round++) {   // the second round records aux_go and aux_ev again
            Bufs b(lens, 41 + round);
            upload_and_verify(check, s, st, b);   // synchronises `stream` alone
            expect_copies(check, "direct", b.total);
        }
        hipstub::drain_all();
        flo::stager_destroy(s);
        hipStreamDestroy(st);
    }
}

// ---- allocation failure -------------------------------------------------------------------------------------------------
void check_allocation() {
    const char *check = "allocation";
    struct Inj {
        int host, event;
        const char *path;   // null: through probe()
    };
    const Inj injs[] = {{2, 0, "ring"}, {3, 0, "ring"}, {4, 0, "ring"}, {0, 2, "ring"}, {2, 0, nullptr}, {3, 0, nullptr}, {4, 0, nullptr}, {0, 2, nullptr}};
    for (const Inj &in : injs) {
        use_path(in.path);
        const hipstub::Counts c0 = hipstub::counts();
        Stager *s = make_stager();
        hipStream_t st = make_stream();
        for (int call = 0; call < 2; call++) {   // the failing upload, then a later one with nothing injected
            Bufs b({9 * MiB + 4, 8 * MiB}, 50 + call);   // three slots' worth; two segments of 16 MiB and more, so the split engages where it is on
            if (call == 0) {
                hipstub::fail_host_malloc(in.host);
                hipstub::fail_event_create(in.event);
            }
            std::string err;
            const int rc = flo::stager_upload(s, b.segs(), st, err);
            hipstub::fail_host_malloc(0);
            hipstub::fail_event_create(0);
            b.scribble_sources();
            hipStreamSynchronize(st);
            if (call == 0 && in.path && rc == 0) fail(check, "the upload whose ring could not be made returned 0", in.host, in.event);
            if (rc != 0 && err.empty()) fail(check, "a failed upload left no message", in.host, in.event);
            if (rc == 0) b.verify(check);   // works, or fails cleanly
        }
        if (!in.path && strcmp(flo::stager_upload_choice(s, nullptr, nullptr), "pageable-direct"))
            fail(check, "the probe did not fall back to the pageable path when the ring could not be made", in.host, in.event);
        flo::stager_destroy(s);
        hipStreamDestroy(st);
        const hipstub::Counts c1 = hipstub::counts();
        if (c1.host_live != c0.host_live || c1.events_live != c0.events_live || c1.dev_live != c0.dev_live || c1.streams_live != c0.streams_live)
            fail(check, "stager_destroy left pinned blocks or events behind", c1.host_live - c0.host_live, c1.events_live - c0.events_live);
        if (c1.violations != c0.violations) fail(check, "something was released twice", in.host, in.event);
    }
}

// ---- worker pool --------------------------------------------------------------------------------------------------------
void check_worker_pool() {
    const char *check = "worker pool";
    use_path("ring");
    Stager *s = make_stager();
    hipStream_t st = make_stream();
    {
        Bufs b({9 * MiB}, 60);   // makes the ring and with it the workers
        upload_and_verify(check, s, st, b);
    }
    const std::vector<std::vector<size_t>> shapes{{}, {1000}, {kPiece - 1}, {kPiece}, {kPiece + 1}, std::vector<size_t>(20, 100 << 10),
                                                  {MiB + 1, 2 * MiB - 1, MiB}, {0, 2 * kPiece + 1, 7, 0, kPiece - 1, 3 * kPiece, 1}};
    for (int call = 0; call < 200; call++) {
        std::vector<size_t> lens = shapes[(size_t)call % shapes.size()];
        for (size_t &n : lens)
            if (n) n += (size_t)(call / (int)shapes.size()) % 3;   // (kPiece - 1, kPiece and kPiece + 1 each arrive in several positions)
        std::vector<std::vector<char>> src, dst;
        std::vector<UploadSeg> segs;
        for (size_t i = 0; i < lens.size(); i++) {
            src.emplace_back(lens[i] + 1);
            dst.emplace_back(lens[i] + 1, (char)0xCC);
            fill_random(src[i].data(), lens[i], 7000 + (uint64_t)call * 16 + i);
            src[i][lens[i]] = 0x55;
        }
        for (size_t i = 0; i < lens.size(); i++) segs.push_back({dst[i].data(), src[i].data(), lens[i]});
        flo::stager_memcpy_many(s, segs);
        for (size_t i = 0; i < lens.size(); i++)
            if (memcmp(dst[i].data(), src[i].data(), lens[i]) || dst[i][lens[i]] != (char)0xCC) fail(check, "a copy differs from its source, or ran past its end", call, i);
    }
    flo::stager_destroy(s);
    hipStreamDestroy(st);
}

}  // namespace

int main() {
    const char *e = getenv("FLO_UPLOAD_THREADS");
    const bool split = g_split = e && atoi(e) >= 2;
    for (int eager = 0; eager < 2; eager++) {
        g_policy = eager ? "eager" : "lazy";
        hipstub::set_eager(eager != 0);
        const struct {
            const char *name;
            void (*run)();
        } checks[] = {{"path", check_paths}, {"small limit", check_small_limit}, {"table", check_table}, {"slot reuse", check_slot_reuse},
                      {"shutdown", check_shutdown}, {"split", check_split}, {"allocation", check_allocation}, {"worker pool", check_worker_pool}};
        for (const auto &c : checks) {
            // with the split switch set only what reaches upload_direct above 16 MiB runs again: the ring and the pool do not read it
            if (split ? (c.run == check_small_limit || c.run == check_slot_reuse || c.run == check_shutdown || c.run == check_worker_pool) : c.run == check_split) continue;
            const auto t0 = std::chrono::steady_clock::now();
            c.run();
            printf("%s, %s: %.2f s\n", c.name, g_policy, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        hipstub::drain_all();
        const hipstub::Counts c = hipstub::counts();
        if (c.host_live || c.dev_live || c.events_live || c.streams_live) fail("end", "blocks, events or streams were never released", c.host_live + c.dev_live, c.events_live + c.streams_live);
        if (c.violations) fail("end", "the runtime model counted violations", c.violations);
    }
    use_path(nullptr);
    const hipstub::Counts c = hipstub::counts();
    printf("%s: %s, both policies; %llu pinned blocks, %llu events, %llu streams made and released\n", g_failures ? "FAILED" : "ok",
           split ? "direct, ring and split paths" : "direct and ring paths", c.host_mallocs, c.events_made, c.streams_made);
    return g_failures ? 1 : 0;
}
