// runtime.hip -- process-wide device resources (runtime.h): the dynamic-LDS
// attribute, the per-launch scratch cache and the helper-stream pool.
#include "runtime.h"

#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace tg {

int lds_attr(const void* fn, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;   // (kernel, device)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return TG_EHIP;
    std::lock_guard<std::mutex> g(mu);
    if (done.count({fn, dev})) return TG_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return TG_EHIP;
    done.insert({fn, dev});
    return TG_OK;
}

// Per-launch scratch (stream_alloc / stream_free): a process-wide
// list of device buffers, each free for reuse once the event recorded behind
// its last launch has completed.  A buffer released on a stream is taken
// again at once only by the next launch on that same stream handle -- never
// through hipStreamPerThread, whose handle names a different stream in each
// thread -- and that launch's stream also waits for
// the buffer's event, so a handle that a destroyed stream left behind and a
// new stream took over cannot reuse a buffer whose work is still pending
// (on the stream that recorded the event the wait orders
// nothing new).  So memory is bounded by the launches in flight, not by the
// streams a caller has ever used.  (The device memory pool of
// hipMallocAsync measured 4.7 MB more per stream used, without reuse across
// streams: profiles/r05/r5b.)  Idle buffers are freed by tg_scratch_trim,
// and by stream_alloc itself once the cache holds more than kScratchHigh
// bytes.
namespace {
struct ScratchBuf {
    void* p = nullptr;
    size_t cap = 0;
    int dev = -1;
    hipEvent_t done = nullptr;   // recorded behind the buffer's last launch
    hipStream_t last = nullptr;  // the stream of that launch
    bool busy = false;           // between stream_alloc and stream_free
};
std::mutex g_scratch_mu;
std::vector<ScratchBuf>& scratch_list() {
    static std::vector<ScratchBuf>* v = new std::vector<ScratchBuf>();   // outlives static teardown
    return *v;
}
// hipStreamPerThread names a different stream in each thread.  The null
// stream does not: this library is built without per-thread default
// streams, so 0 is the device's legacy default stream, one per device (and
// buffers and helpers are kept per device).  Round 6 treated 0 as
// per-thread too: every key-table batch on the default stream then created a
// new helper stream while the last one's work was in flight (config 4
// 657 -> 547 GiB/s, profiles/r06/f2/bench_c4.json).
bool per_thread_handle(hipStream_t s) { return s == hipStreamPerThread; }
constexpr size_t kScratchHigh = (size_t)8 << 30;

// Unlinks idle buffers whose last launch has completed until the cache holds
// at most ``keep`` bytes, largest first (g_scratch_mu held), and returns them.
std::vector<ScratchBuf> unlink_idle(size_t keep) {
    auto& v = scratch_list();
    std::vector<ScratchBuf> out;
    size_t total = 0;
    for (const auto& b : v) total += b.cap;
    while (total > keep) {
        size_t best = v.size();
        for (size_t i = 0; i < v.size(); ++i) {
            const ScratchBuf& b = v[i];
            if (b.busy || (b.done && hipEventQuery(b.done) != hipSuccess)) continue;
            if (best == v.size() || b.cap > v[best].cap) best = i;
        }
        if (best == v.size()) break;   // everything left is in use
        total -= v[best].cap;
        out.push_back(v[best]);
        v.erase(v.begin() + (std::ptrdiff_t)best);
    }
    return out;
}

// Frees what unlink_idle() took out, with g_scratch_mu released: hipFree may
// synchronise the device, and no other thread should wait for that to take
// or return scratch.
void free_unlinked(const std::vector<ScratchBuf>& bufs) {
    for (const ScratchBuf& b : bufs) {
        int cur = 0;
        const bool switch_dev = hipGetDevice(&cur) == hipSuccess && cur != b.dev;
        if (switch_dev) (void)hipSetDevice(b.dev);
        (void)hipFree(b.p);
        if (b.done) (void)hipEventDestroy(b.done);
        if (switch_dev) (void)hipSetDevice(cur);
    }
}
}  // namespace

int stream_alloc(void** p, size_t bytes, hipStream_t s) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return TG_EHIP;
    if (!bytes) bytes = 1;
    std::unique_lock<std::mutex> g(g_scratch_mu);
    auto& v = scratch_list();
    ScratchBuf* pick = nullptr;
    bool pick_pending = false;
    for (auto& b : v) {
        if (b.busy || b.dev != dev || b.cap < bytes) continue;
        const bool complete = !b.done || hipEventQuery(b.done) == hipSuccess;
        const bool ordered = b.last == s && !per_thread_handle(s);
        if (complete || ordered) {
            if (!pick || b.cap < pick->cap) {
                pick = &b;
                pick_pending = !complete;
            }
        }
    }
    if (pick) {
        if (pick_pending && hipStreamWaitEvent(s, pick->done, 0) != hipSuccess) return TG_EHIP;
        pick->busy = true;
        *p = pick->p;
        return TG_OK;
    }
    size_t total = 0;
    for (const auto& b : v) total += b.cap;
    if (total + bytes > kScratchHigh) {
        const auto victims = unlink_idle(kScratchHigh > bytes ? kScratchHigh - bytes : 0);
        g.unlock();
        free_unlinked(victims);
        g.lock();
    }
    ScratchBuf nb;
    nb.cap = bytes < (1u << 20) ? (size_t)1 << 20 : (bytes + 0xfffff) & ~(size_t)0xfffff;
    nb.dev = dev;
    nb.busy = true;
    if (hipMalloc(&nb.p, nb.cap) != hipSuccess) return TG_EHIP;
    if (hipEventCreateWithFlags(&nb.done, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(nb.p);
        return TG_EHIP;
    }
    v.push_back(nb);
    *p = nb.p;
    return TG_OK;
}

void scratch_totals(uint64_t* bytes, uint64_t* buffers) {
    std::lock_guard<std::mutex> g(g_scratch_mu);
    *bytes = 0;
    *buffers = scratch_list().size();
    for (const auto& b : scratch_list()) *bytes += b.cap;
}

// The event is recorded first: only once the record has succeeded is the
// buffer reusable.  If it fails the buffer stays busy (leaked, never handed
// out behind a stale event) and the caller gets TG_EHIP.
int stream_free(void* p, hipStream_t s) {
    std::lock_guard<std::mutex> g(g_scratch_mu);
    for (auto& b : scratch_list()) {
        if (b.p != p) continue;
        if (hipEventRecord(b.done, s) != hipSuccess) return TG_EHIP;
        b.busy = false;
        b.last = s;
        return TG_OK;
    }
    return TG_EINVAL;
}

// Helper streams (helper_fork / helper_join): a process-wide pool.
// A launch that runs a second kernel beside its main one (the key-table
// short records, aes_gcm_bs8.hip launch_kt) takes a helper of its device and
// priority class that is idle -- its last join has completed -- or that
// its own stream used last, so independent callers never queue behind each
// other's helper work (round 5 had one helper per device shared
// by every caller).  A caller at raised priority gets a helper at its own
// priority; any other caller one at the lowest priority (the short records
// fill the CUs the long kernel's tail leaves idle, profiles/r05/r5z/).
namespace {
struct HelperStream {
    hipStream_t h = nullptr;
    int dev = -1;
    int prio = 0;
    hipEvent_t fork = nullptr, join = nullptr;
    hipStream_t last = nullptr;
    bool busy = false;
};
std::mutex g_helper_mu;
std::vector<HelperStream>& helper_list() {
    static std::vector<HelperStream>* v = new std::vector<HelperStream>();
    return *v;
}
}  // namespace

int helper_fork(hipStream_t s, hipStream_t* out) {
    *out = nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return TG_EHIP;
    // the caller's stream on another device than the current one: no helper
    hipDevice_t sd = 0;
    if (hipStreamGetDevice(s, &sd) == hipSuccess && (int)sd != dev) return TG_OK;
    int least = 0, greatest = 0, sp = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;
    if (hipStreamGetPriority(s, &sp) != hipSuccess) sp = 0;
    // priorities: lower numbers run first; 0 is the default
    const int prio = sp < 0 && least != greatest ? sp : least;
    std::lock_guard<std::mutex> g(g_helper_mu);
    auto& v = helper_list();
    HelperStream* pick = nullptr;
    for (auto& x : v) {
        if (x.busy || x.dev != dev || x.prio != prio) continue;
        if ((x.last == s && !per_thread_handle(s)) || hipEventQuery(x.join) == hipSuccess) {
            pick = &x;
            break;
        }
    }
    if (!pick) {
        HelperStream x;
        x.dev = dev;
        x.prio = prio;
        if (hipStreamCreateWithPriority(&x.h, hipStreamNonBlocking, prio) != hipSuccess) return TG_EHIP;
        if (hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&x.join, hipEventDisableTiming) != hipSuccess) {
            if (x.fork) (void)hipEventDestroy(x.fork);
            (void)hipStreamDestroy(x.h);
            return TG_EHIP;
        }
        v.push_back(x);
        pick = &v.back();
    }
    if (hipEventRecord(pick->fork, s) != hipSuccess || hipStreamWaitEvent(pick->h, pick->fork, 0) != hipSuccess)
        return TG_EHIP;
    pick->busy = true;
    *out = pick->h;
    return TG_OK;
}

int helper_join(hipStream_t h, hipStream_t s) {
    std::lock_guard<std::mutex> g(g_helper_mu);
    for (auto& x : helper_list()) {
        if (x.h != h || !x.busy) continue;
        // on failure the helper stays busy: never handed out behind a join
        // event that does not cover its work
        if (hipEventRecord(x.join, h) != hipSuccess || hipStreamWaitEvent(s, x.join, 0) != hipSuccess)
            return TG_EHIP;
        x.busy = false;
        x.last = s;
        return TG_OK;
    }
    return TG_EINVAL;
}

void helper_totals(uint64_t* streams, uint64_t* busy) {
    std::lock_guard<std::mutex> g(g_helper_mu);
    *streams = helper_list().size();
    *busy = 0;
    for (const auto& x : helper_list()) *busy += x.busy;
}

// Frees every idle helper whose work has completed, and idle scratch
// buffers down to ``keep`` bytes (tg_scratch_trim).
void scratch_trim(size_t keep) {
    std::vector<ScratchBuf> victims;
    {
        std::lock_guard<std::mutex> g(g_scratch_mu);
        victims = unlink_idle(keep);
    }
    free_unlinked(victims);
    std::lock_guard<std::mutex> g(g_helper_mu);
    auto& v = helper_list();
    for (size_t i = 0; i < v.size();) {
        HelperStream& x = v[i];
        if (x.busy || hipEventQuery(x.join) != hipSuccess || hipStreamQuery(x.h) != hipSuccess) {
            ++i;
            continue;
        }
        (void)hipStreamDestroy(x.h);
        (void)hipEventDestroy(x.fork);
        (void)hipEventDestroy(x.join);
        v.erase(v.begin() + (std::ptrdiff_t)i);
    }
}

}  // namespace tg
