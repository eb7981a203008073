// The device pool (flo_amd/csrc/devpool.cpp) under eight host threads, on the CPU: the pool is one object for all the
// contexts of a process, so every context's thread meets the others in it. Built by tests/test_devpool_threads_cpu.py with
// -fsanitize=thread against tests/native/hipstub (the five runtime calls the pool needs are defined below on malloc).
//
// What is checked:
//   * the size classes at their edges (below 256 B, around 64 KiB, the eighth-octave steps), single-threaded, by what the
//     driver is asked for;
//   * eight threads allocate, write, verify and free blocks of those sizes, with flo_debug_pool_fill toggled and
//     pool_trim called beside them: every byte a thread wrote into a block is still its own when it frees the block (a
//     block in two hands at once shows as a foreign byte, and as a data race to the sanitizer);
//   * blocks above kMaxCachedBlock go straight back to the driver, and the cache never holds more than kMaxCachedTotal:
//     the threads free 2.6 GiB of large blocks between them;
//   * an allocation the driver refuses for lack of memory succeeds once the pool has given its cache back;
//   * at the end every block the driver handed out came back to it exactly once.
// Blocks of 160 KiB and more are written at both ends and one byte per 256 KiB between, and so is the stub's memset of them: their pages are
// never all resident.
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "devpool.hpp"

extern "C" int flo_debug_pool_fill(int byte);

// ---- the driver: malloc, and a ledger of what is out ----------------------------------------------------------------
namespace {
std::mutex d_mu;
std::unordered_map<void *, size_t> d_out;   // handed out by hipMalloc and not yet back
size_t d_out_bytes = 0, d_out_peak = 0, d_last_malloc = 0;
unsigned long long d_mallocs = 0, d_frees = 0, d_refused = 0;
std::atomic<size_t> d_cap{(size_t)64 << 30};   // hipMalloc refuses what would take the bytes that are out beyond this
std::atomic<int> g_failures{0};

void fail(const char *what, unsigned long long a = 0, unsigned long long b = 0) {
    fprintf(stderr, "FAIL: %s (%llu, %llu)\n", what, a, b);
    g_failures.fetch_add(1);
}
constexpr size_t kSparseFrom = (size_t)160 << 10, kPage = 4096, kStride = 64 * kPage;
}  // namespace

hipError_t hipGetDevice(int *device) {
    *device = 0;
    return hipSuccess;
}
hipError_t hipMalloc(void **ptr, size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(d_mu);
        if (d_out_bytes + bytes > d_cap.load()) {
            d_refused++;
            *ptr = nullptr;
            return hipErrorOutOfMemory;
        }
    }
    void *p = malloc(bytes);
    if (!p) return hipErrorOutOfMemory;
    std::lock_guard<std::mutex> lk(d_mu);
    if (!d_out.emplace(p, bytes).second) fail("the driver handed out a block that is out");
    d_out_bytes += bytes;
    if (d_out_bytes > d_out_peak) d_out_peak = d_out_bytes;
    d_last_malloc = bytes;
    d_mallocs++;
    *ptr = p;
    return hipSuccess;
}
hipError_t hipFree(void *ptr) {
    if (!ptr) return hipSuccess;
    {
        std::lock_guard<std::mutex> lk(d_mu);
        auto it = d_out.find(ptr);
        if (it == d_out.end()) {
            fail("hipFree of a block that is not out (freed twice, or never allocated)");
            return hipSuccess;
        }
        d_out_bytes -= it->second;
        d_out.erase(it);
        d_frees++;
    }
    free(ptr);
    return hipSuccess;
}
hipError_t hipMemset(void *dst, int value, size_t bytes) {
    uint8_t *p = (uint8_t *)dst;
    if (bytes < kSparseFrom) {
        memset(p, value, bytes);
        return hipSuccess;
    }
    memset(p, value, kPage);
    memset(p + bytes - kPage, value, kPage);
    for (size_t i = kPage; i < bytes - kPage; i += kStride) p[i] = (uint8_t)value;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }

// ---- a block in a thread's hands ------------------------------------------------------------------------------------
namespace {
struct Held {
    uint8_t *p;
    size_t bytes;
    uint8_t tag;
};

template <class F>
void each_written(size_t bytes, F f) {   // every byte of a small block; both ends (4 KiB each) and one byte per 256 KiB of a large one
    if (bytes < kSparseFrom) {
        for (size_t i = 0; i < bytes; i++) f(i);
        return;
    }
    for (size_t i = 0; i < kPage; i++) f(i);
    for (size_t i = kPage; i < bytes - kPage; i += kStride) f(i);
    for (size_t i = bytes - kPage; i < bytes; i++) f(i);
}
void write_block(const Held &h) {
    each_written(h.bytes, [&](size_t i) { h.p[i] = (uint8_t)(h.tag + i * 7); });
}
bool verify_block(const Held &h) {
    bool ok = true;
    each_written(h.bytes, [&](size_t i) { ok = ok && h.p[i] == (uint8_t)(h.tag + i * 7); });
    return ok;
}

bool take(std::vector<Held> &held, size_t bytes, uint8_t tag) {
    void *p = nullptr;
    hipError_t e = flo::pool_alloc(&p, bytes);
    if (e != hipSuccess || !p) return false;
    Held h{(uint8_t *)p, bytes, tag};
    write_block(h);
    held.push_back(h);
    return true;
}
void give_back(std::vector<Held> &held, size_t at) {
    Held h = held[at];
    held.erase(held.begin() + at);
    if (!verify_block(h)) fail("a block's bytes changed while its owner held it", h.bytes, h.tag);
    flo::pool_free(h.p);
}

// the sizes at which the pool takes another path
const size_t kSizes[] = {1, 255, 256, 257, 511, 512, 513, 4096, 65535, 65536, 65537,            // 256 B steps, and their end
                         (72u << 10) - 1, 72u << 10, (72u << 10) + 1, (80u << 10) + 1,            // eighth-octave steps above 64 KiB
                         (128u << 10) - 1, 128u << 10, (128u << 10) + 1, (144u << 10) + 1,        // the next octave
                         (1u << 20) - 1, (1u << 20) + 1, (3u << 20) + 5};
constexpr int kThreads = 8, kRounds = 1000, kHold = 6;
constexpr size_t kLarge = (size_t)110 << 20;   // class 112 MiB: cached; 8 threads x 3 of them pass kMaxCachedTotal

std::mutex m_mu;
std::condition_variable m_cv;
int m_arrived = 0;
void all_hold_theirs() {   // returns once all kThreads threads have called it
    std::unique_lock<std::mutex> lk(m_mu);
    if (++m_arrived == kThreads) m_cv.notify_all();
    else m_cv.wait(lk, [] { return m_arrived == kThreads; });
}

void worker(int t) {
    std::vector<Held> held;
    uint32_t rng = 12345u + 977u * (uint32_t)t;
    auto next = [&] { return rng = rng * 1664525u + 1013904223u; };
    for (int r = 0; r < kRounds; r++) {
        const size_t bytes = kSizes[(next() >> 8) % (sizeof kSizes / sizeof *kSizes)];
        if (!take(held, bytes, (uint8_t)(t * 32 + r))) fail("pool_alloc failed", bytes);
        if (held.size() > (size_t)kHold) give_back(held, (next() >> 8) % held.size());
        if (t == 0 && r % 64 == 0) flo_debug_pool_fill((r / 64) % 3 == 0 ? -1 : (r / 64) % 3 == 1 ? 0x7F : 0xFF);
        if (t == 1 && r % 100 == 50) flo::pool_trim();
        if (t >= 2 && r % 500 == 250) {   // above kMaxCachedBlock: never cached
            void *p = nullptr;
            if (flo::pool_alloc(&p, flo::kMaxCachedBlock + 1 + (size_t)t) != hipSuccess) fail("pool_alloc of a block above kMaxCachedBlock failed");
            else flo::pool_free(p);
        }
    }
    while (!held.empty()) give_back(held, held.size() - 1);
    // the large blocks: every thread holds three before any is freed, so 2.6 GiB come back and not all of it may be cached
    for (int k = 0; k < 3; k++)
        if (!take(held, kLarge + (size_t)(t * 3 + k), (uint8_t)(t * 16 + k))) fail("pool_alloc of a large block failed");
    all_hold_theirs();
    while (!held.empty()) give_back(held, 0);
}

size_t driver_asked_for(size_t bytes) {
    void *p = nullptr;
    if (flo::pool_alloc(&p, bytes) != hipSuccess) return 0;
    size_t got;
    {
        std::lock_guard<std::mutex> lk(d_mu);
        got = d_last_malloc;
    }
    flo::pool_free(p);
    flo::pool_trim();   // (so that the next size of the same class goes to the driver again)
    return got;
}
}  // namespace

int main() {
    // 1. the classes, by what reaches the driver
    const struct {
        size_t bytes, cls;
    } classes[] = {{0, 256}, {1, 256}, {255, 256}, {256, 256}, {257, 512}, {65535, 65536}, {65536, 65536},
                   {65537, 72u << 10}, {72u << 10, 72u << 10}, {(72u << 10) + 1, 80u << 10}, {(128u << 10) - 1, 128u << 10},
                   {(128u << 10) + 1, 144u << 10}, {(size_t)(3u << 20) + 5, (size_t)(3u << 20) + (256u << 10)},
                   {flo::kMaxCachedBlock, flo::kMaxCachedBlock}, {flo::kMaxCachedBlock + 1, flo::kMaxCachedBlock + (flo::kMaxCachedBlock >> 3)}};
    for (auto &c : classes) {
        const size_t got = driver_asked_for(c.bytes);
        if (got != c.cls) fail("size class", c.bytes, got);
    }
    // a filled block arrives filled over its whole class, an unfilled one as it was left
    flo_debug_pool_fill(0x7F);
    {
        void *p = nullptr;
        if (flo::pool_alloc(&p, 300) != hipSuccess) return 2;
        for (int i = 0; i < 512; i++)
            if (((uint8_t *)p)[i] != 0x7F) {
                fail("the fill does not cover the class", i);
                break;
            }
        memset(p, 0x11, 512);
        flo::pool_free(p);
        flo_debug_pool_fill(-1);
        void *q = nullptr;
        if (flo::pool_alloc(&q, 400) != hipSuccess) return 2;
        if (q != p || ((uint8_t *)q)[0] != 0x11) fail("a freed block of the class was not handed out again as it was left");
        flo::pool_free(q);
    }
    flo::pool_trim();
    {
        std::lock_guard<std::mutex> lk(d_mu);
        if (!d_out.empty()) fail("blocks are out after pool_trim", d_out.size());
    }

    // 2. eight threads
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; t++) th.emplace_back(worker, t);
    for (auto &x : th) x.join();
    flo_debug_pool_fill(-1);
    size_t cached;
    unsigned long long frees_before;
    {
        std::lock_guard<std::mutex> lk(d_mu);
        cached = d_out_bytes;   // nothing is in a thread's hands any more: what is out is what the pool caches
        frees_before = d_frees;
        if (d_out_peak <= flo::kMaxCachedTotal) fail("the threads never held more than kMaxCachedTotal", d_out_peak);
    }
    if (cached > flo::kMaxCachedTotal) fail("the pool caches more than kMaxCachedTotal", cached);
    if (cached + ((size_t)112 << 20) <= flo::kMaxCachedTotal) fail("the cache was not filled to its limit by the large blocks", cached);

    // 3. the driver refuses: the pool gives its cache back and tries once more
    d_cap.store(cached + ((size_t)64 << 20));
    {
        void *p = nullptr;
        if (flo::pool_alloc(&p, (size_t)100 << 20) != hipSuccess) fail("pool_alloc did not recover from hipErrorOutOfMemory");
        {
            std::lock_guard<std::mutex> lk(d_mu);
            if (d_refused != 1) fail("the driver was expected to refuse exactly once", d_refused);
            if (d_frees == frees_before) fail("the cache was not given back");
        }
        flo::pool_free(p);
    }
    d_cap.store((size_t)64 << 30);

    // 4. everything goes back exactly once
    flo::pool_trim();
    {
        std::lock_guard<std::mutex> lk(d_mu);
        if (!d_out.empty() || d_out_bytes) fail("blocks never returned to the driver", d_out.size(), d_out_bytes);
        if (d_mallocs != d_frees) fail("hipMalloc and hipFree counts differ", d_mallocs, d_frees);
        printf("%s: %llu blocks from the driver, %llu returned, peak %zu MiB out, %zu MiB cached after the large blocks\n",
               g_failures.load() ? "FAILED" : "ok", d_mallocs, d_frees, d_out_peak >> 20, cached >> 20);
    }
    return g_failures.load() ? 1 : 0;
}
