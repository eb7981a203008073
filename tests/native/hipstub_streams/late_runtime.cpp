// A deferred-execution stand-in for the HIP runtime, on the CPU: the device runs late. Declared in hip/hip_runtime.h
// beside this file; linked into tests/native/stager_paths_test.cpp only.
//
//   * A stream is a FIFO of ops: copy, memset, event marker, wait for a marker, gate, nop.
//   * hipMemcpyAsync from memory that hipHostMalloc handed out queues (dst, src, bytes) and copies NOTHING: the bytes are
//     read when the op runs, as a copy engine reads pinned memory. From any other host memory the source is snapshotted at
//     the call (the runtime's pageable staging) and the write to dst is queued.
//   * hipEventRecord queues a marker; hipStreamWaitEvent queues a dependency on the marker that was recorded last at that
//     moment; hipEventSynchronize and hipStreamSynchronize run ops in stream order up to the marker, or to the end, and
//     resolve dependencies first (by running the other stream up to the marker waited for).
//   * A gate holds a stream until a host thread opens it; a synchronise that reaches a closed gate blocks.
//   * Two policies (set_eager): lazy runs nothing until something synchronises on it; eager runs an op as soon as it is at
//     the head of its stream with its dependencies met. A missing wait shows under one or the other.
//   * "Device memory" is malloc with kGuard guard bytes on both sides; a copy or memset must lie inside one block.
//   * hipFree and hipHostFree overwrite the block with kPoison before they release it, and a block that queued ops still
//     name is a violation (the block is then kept, poisoned, so that the late op copies poison and not freed memory).
//   * hipHostMalloc and hipEventCreateWithFlags can be made to fail at their n-th call.
//   * hipStreamDestroy and hipEventDestroy never block: the objects live on until the process ends, so queued ops that
//     name them stay valid (the runtime releases them when their work has completed). A destroyed stream's ops still run.
// One mutex guards everything; ops run under it.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <vector>

struct hipstubEvent {
    unsigned long long issued = 0, done = 0;   // markers queued / markers passed
    hipstubStream *last_stream = nullptr;       // where the last marker was queued,
    unsigned long long last_op = 0;             // and its op id there
    bool live = true;
};

namespace {
enum Kind { COPY, MEMSET, MARK, WAIT, GATE, NOP };
struct Op {
    Kind kind = NOP;
    unsigned long long id = 0;
    char *dst = nullptr;
    const char *src = nullptr;
    size_t bytes = 0;
    std::shared_ptr<std::vector<char>> snap;   // pageable source, taken at the call
    bool pinned = false;
    int value = 0;
    hipstubEvent *ev = nullptr;
    unsigned long long seq = 0;                 // MARK: its number; WAIT: the number waited for
    hipstubStream *from = nullptr;              // WAIT: the stream that holds the marker, and its op id there
    unsigned long long from_op = 0;
    int gate = 0;
};
}  // namespace

struct hipstubStream {
    std::deque<Op> q;
    unsigned long long next_id = 1;
    bool live = true;
};

namespace {
std::mutex g_mu;
std::condition_variable g_cv;
bool g_eager = false;
std::map<const char *, size_t> g_host, g_dev;   // live blocks: user pointer -> bytes
std::vector<std::unique_ptr<hipstubStream>> g_streams;
std::vector<std::unique_ptr<hipstubEvent>> g_events;
std::set<int> g_closed_gates;
int g_next_gate = 1, g_gate_waiters = 0;
int g_fail_host = 0, g_fail_event = 0;
hipstub::Counts g_c{};

void violation(const char *what, unsigned long long a = 0, unsigned long long b = 0) {
    fprintf(stderr, "MODEL: %s (%llu, %llu)\n", what, a, b);
    g_c.violations++;
}

// the live block that holds [p, p + bytes), or null
const char *block_of(const std::map<const char *, size_t> &m, const char *p, size_t bytes) {
    auto it = m.upper_bound(p);
    if (it == m.begin()) return nullptr;
    --it;
    return p + bytes <= it->first + it->second ? it->first : nullptr;
}

void execute(const Op &op) {
    switch (op.kind) {
        case COPY:
            if (!block_of(g_dev, op.dst, op.bytes)) {
                violation("a copy's destination is not inside one live device block", op.bytes);
                return;
            }
            if (op.pinned && !block_of(g_host, op.src, op.bytes)) violation("a copy ran from pinned memory that had been freed", op.bytes);
            memcpy(op.dst, op.pinned ? op.src : op.snap->data(), op.bytes);
            g_c.copies_run++;
            g_c.copied_bytes += op.bytes;
            break;
        case MEMSET:
            if (!block_of(g_dev, op.dst, op.bytes)) {
                violation("a memset's destination is not inside one live device block", op.bytes);
                return;
            }
            memset(op.dst, op.value, op.bytes);
            break;
        case MARK:
            if (op.ev->done < op.seq) op.ev->done = op.seq;
            break;
        default:
            break;
    }
}

bool ready(const Op &op) {
    if (op.kind == WAIT) return op.ev->done >= op.seq;
    if (op.kind == GATE) return !g_closed_gates.count(op.gate);
    return true;
}

// eager: run whatever can run, anywhere, until nothing can
void pump() {
    if (!g_eager) return;
    for (bool progress = true; progress;) {
        progress = false;
        for (size_t i = 0; i < g_streams.size(); i++) {
            hipstubStream *s = g_streams[i].get();
            while (!s->q.empty() && ready(s->q.front())) {
                Op op = std::move(s->q.front());
                s->q.pop_front();
                execute(op);
                progress = true;
            }
        }
    }
}

// run `s` in order until the op with id `upto` has run; blocks at a closed gate (the lock is released meanwhile)
void run_to(std::unique_lock<std::mutex> &lk, hipstubStream *s, unsigned long long upto) {
    while (!s->q.empty() && s->q.front().id <= upto) {
        const Op &head = s->q.front();
        if (head.kind == WAIT && head.ev->done < head.seq) {
            hipstubStream *from = head.from;
            const unsigned long long from_op = head.from_op;
            hipstubEvent *ev = head.ev;
            const unsigned long long seq = head.seq;
            run_to(lk, from, from_op);
            if (ev->done < seq) {
                violation("a marker that a stream waits for is queued nowhere", seq);
                ev->done = seq;
            }
            continue;   // (the queue may have changed while a gate was waited for)
        }
        if (head.kind == GATE && g_closed_gates.count(head.gate)) {
            const int id = head.gate;
            g_gate_waiters++;
            g_cv.wait(lk, [&] { return !g_closed_gates.count(id); });
            g_gate_waiters--;
            continue;
        }
        Op op = std::move(s->q.front());
        s->q.pop_front();
        execute(op);
    }
    pump();
}

void push(hipstubStream *s, Op op) {
    op.id = s->next_id++;
    s->q.push_back(std::move(op));
}

bool names(const Op &op, const char *p, size_t bytes) {
    if (op.kind == COPY && op.pinned && op.src + op.bytes > p && op.src < p + bytes) return true;
    if ((op.kind == COPY || op.kind == MEMSET) && op.dst + op.bytes > p && op.dst < p + bytes) return true;
    return false;
}
bool queued_ops_name(const char *p, size_t bytes) {
    for (auto &s : g_streams)
        for (const Op &op : s->q)
            if (names(op, p, bytes)) return true;
    return false;
}
}  // namespace

hipError_t hipGetDevice(int *device) {
    *device = 0;
    return hipSuccess;
}
hipError_t hipSetDevice(int device) { return device == 0 ? hipSuccess : hipErrorInvalidValue; }

hipError_t hipMalloc(void **ptr, size_t bytes) {
    char *raw = (char *)malloc(bytes + 2 * hipstub::kGuard);
    if (!raw) return hipErrorOutOfMemory;
    memset(raw, hipstub::kGuardByte, hipstub::kGuard);
    memset(raw + hipstub::kGuard + bytes, hipstub::kGuardByte, hipstub::kGuard);
    std::lock_guard<std::mutex> lk(g_mu);
    g_dev[raw + hipstub::kGuard] = bytes;
    g_c.dev_mallocs++;
    *ptr = raw + hipstub::kGuard;
    return hipSuccess;
}

static bool guards_intact_locked(const char *p, size_t bytes) {
    for (size_t i = 0; i < hipstub::kGuard; i++)
        if ((unsigned char)p[-(ptrdiff_t)hipstub::kGuard + (ptrdiff_t)i] != hipstub::kGuardByte || (unsigned char)p[bytes + i] != hipstub::kGuardByte) return false;
    return true;
}

hipError_t hipFree(void *ptr) {
    if (!ptr) return hipSuccess;
    char *p = (char *)ptr;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_dev.find(p);
    if (it == g_dev.end()) {
        violation("hipFree of a block that is not out (freed twice, or never allocated)");
        return hipErrorInvalidValue;
    }
    const size_t bytes = it->second;
    if (!guards_intact_locked(p, bytes)) violation("guard bytes of a device block were overwritten", bytes);
    g_dev.erase(it);
    g_c.dev_frees++;
    memset(p, hipstub::kPoison, bytes);
    if (queued_ops_name(p, bytes)) violation("hipFree of a block that queued ops still write", bytes);   // kept: the late op finds memory
    else free(p - hipstub::kGuard);
    return hipSuccess;
}

hipError_t hipHostMalloc(void **ptr, size_t bytes, unsigned) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_fail_host && --g_fail_host == 0) {
        *ptr = nullptr;
        return hipErrorOutOfMemory;
    }
    char *p = (char *)malloc(bytes ? bytes : 1);
    if (!p) return hipErrorOutOfMemory;
    g_host[p] = bytes;
    g_c.host_mallocs++;
    *ptr = p;
    return hipSuccess;
}

hipError_t hipHostFree(void *ptr) {
    if (!ptr) return hipSuccess;
    char *p = (char *)ptr;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_host.find(p);
    if (it == g_host.end()) {
        violation("hipHostFree of a block that is not out (freed twice, or never allocated)");
        return hipErrorInvalidValue;
    }
    const size_t bytes = it->second;
    g_host.erase(it);
    g_c.host_frees++;
    memset(p, hipstub::kPoison, bytes);
    if (queued_ops_name(p, bytes)) violation("hipHostFree of a pinned block that queued copies still read", bytes);   // kept, poisoned
    else free(p);
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_streams.emplace_back(new hipstubStream());
    g_c.streams_made++;
    *stream = g_streams.back().get();
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!stream || !stream->live) {
        violation("hipStreamDestroy of a stream that is not live");
        return hipErrorInvalidValue;
    }
    stream->live = false;
    g_c.streams_destroyed++;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
    std::unique_lock<std::mutex> lk(g_mu);
    if (!stream || !stream->live) {
        violation("hipStreamSynchronize of a stream that is not live");
        return hipErrorInvalidValue;
    }
    run_to(lk, stream, ~0ull);
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_fail_event && --g_fail_event == 0) {
        *event = nullptr;
        return hipErrorOutOfMemory;
    }
    g_events.emplace_back(new hipstubEvent());
    g_c.events_made++;
    *event = g_events.back().get();
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!event || !event->live) {
        violation("hipEventDestroy of an event that is not live");
        return hipErrorInvalidValue;
    }
    event->live = false;
    g_c.events_destroyed++;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    std::unique_lock<std::mutex> lk(g_mu);
    if (!event || !event->live || !stream || !stream->live) {
        violation("hipEventRecord with an event or a stream that is not live");
        return hipErrorInvalidValue;
    }
    Op op;
    op.kind = MARK;
    op.ev = event;
    op.seq = ++event->issued;
    event->last_stream = stream;
    event->last_op = stream->next_id;
    push(stream, std::move(op));
    pump();
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event) {
    std::unique_lock<std::mutex> lk(g_mu);
    if (!event || !event->live) {
        violation("hipEventSynchronize of an event that is not live");
        return hipErrorInvalidValue;
    }
    if (event->done < event->issued) run_to(lk, event->last_stream, event->last_op);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned) {
    std::unique_lock<std::mutex> lk(g_mu);
    if (!event || !event->live || !stream || !stream->live) {
        violation("hipStreamWaitEvent with an event or a stream that is not live");
        return hipErrorInvalidValue;
    }
    if (!event->issued) return hipSuccess;   // never recorded: nothing to wait for
    Op op;
    op.kind = WAIT;
    op.ev = event;
    op.seq = event->issued;
    op.from = event->last_stream;
    op.from_op = event->last_op;
    push(stream, std::move(op));
    pump();
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    std::unique_lock<std::mutex> lk(g_mu);
    if (kind != hipMemcpyHostToDevice || !stream || !stream->live) {
        violation("hipMemcpyAsync: only host-to-device copies on a live stream are modelled");
        return hipErrorInvalidValue;
    }
    Op op;
    op.kind = COPY;
    op.dst = (char *)dst;
    op.bytes = bytes;
    if (block_of(g_host, (const char *)src, bytes)) {
        op.pinned = true;
        op.src = (const char *)src;
        g_c.pinned_copies++;
    } else {
        op.snap = std::make_shared<std::vector<char>>((const char *)src, (const char *)src + bytes);
        g_c.pageable_copies++;
    }
    push(stream, std::move(op));
    pump();
    return hipSuccess;
}

namespace hipstub {

void set_eager(bool eager) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_eager = eager;
}

int gate(hipStream_t stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    Op op;
    op.kind = GATE;
    op.gate = g_next_gate++;
    g_closed_gates.insert(op.gate);
    const int id = op.gate;
    push(stream, std::move(op));
    return id;
}
void open_gate(int id) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_closed_gates.erase(id);
        pump();
    }
    g_cv.notify_all();
}
int gate_waiters() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_gate_waiters;
}

hipError_t memset_async(void *dst, int value, size_t bytes, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    Op op;
    op.kind = MEMSET;
    op.dst = (char *)dst;
    op.value = value;
    op.bytes = bytes;
    push(stream, std::move(op));
    pump();
    return hipSuccess;
}
hipError_t nop_async(hipStream_t stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    push(stream, Op());
    pump();
    return hipSuccess;
}

void fail_host_malloc(int nth) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_fail_host = nth;
}
void fail_event_create(int nth) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_fail_event = nth;
}

void drain_all() {
    std::unique_lock<std::mutex> lk(g_mu);
    if (!g_closed_gates.empty()) {
        violation("drain_all with a gate closed");
        return;
    }
    for (size_t i = 0; i < g_streams.size(); i++) run_to(lk, g_streams[i].get(), ~0ull);
}

Counts counts() {
    std::lock_guard<std::mutex> lk(g_mu);
    Counts c = g_c;
    c.host_live = g_host.size();
    c.dev_live = g_dev.size();
    c.events_live = (size_t)(g_c.events_made - g_c.events_destroyed);
    c.streams_live = (size_t)(g_c.streams_made - g_c.streams_destroyed);
    return c;
}
void reset_copy_counts() {
    std::lock_guard<std::mutex> lk(g_mu);
    g_c.copies_run = g_c.copied_bytes = g_c.pinned_copies = g_c.pageable_copies = 0;
}
bool guards_intact(const void *p) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_dev.find((const char *)p);
    return it != g_dev.end() && guards_intact_locked(it->first, it->second);
}

}  // namespace hipstub
