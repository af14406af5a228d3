// runtime.h -- process-wide device resources of libtlsgpu (runtime.hip): the
// dynamic-LDS attribute, the per-launch scratch cache, the helper-stream pool
// and the CU count.  Host side only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "tlsgpu.h"

namespace tg {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for ``fn`` on the current
// device, once per (function, device); thread-safe.  0 or TG_EHIP.
int lds_attr(const void* fn, int bytes);

// Per-launch device scratch for launches on stream ``s``: stream_alloc takes
// a buffer of at least ``bytes`` from a process-wide cache (reused once the
// launches that last used it have completed, or at once by the next launch
// on the same stream), stream_free hands it back behind the work queued on
// ``s``.  0, TG_EHIP, or TG_EINVAL for a pointer not from stream_alloc.
int stream_alloc(void** p, size_t bytes, hipStream_t s);
int stream_free(void* p, hipStream_t s);
void scratch_totals(uint64_t* bytes, uint64_t* buffers);   // tg_scratch_info
void scratch_trim(size_t keep);                             // tg_scratch_trim

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

// One launch's scratch: a single stream_alloc buffer, carved front to back.
// take() rounds the running offset up to ``align`` (a power of two, at most
// the 256 bytes hipMalloc aligns the buffer to) and hands out ``bytes`` from
// there; the caller sizes alloc() for the carves it makes.  release() gives
// the buffer back behind the work queued on the stream and returns
// stream_free's status; the destructor does it for early returns.
class Scratch {
  public:
    explicit Scratch(hipStream_t s) : s_(s) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { (void)release(); }
    int alloc(size_t bytes) { return stream_alloc((void**)&base_, bytes, s_); }
    template <class T>
    T* take(size_t bytes, size_t align) {
        off_ = align_up(off_, align);
        T* p = reinterpret_cast<T*>(base_ + off_);
        off_ += bytes;
        return p;
    }
    int release() {
        uint8_t* p = base_;
        base_ = nullptr;
        return p ? stream_free(p, s_) : TG_OK;
    }

  private:
    hipStream_t s_;
    uint8_t* base_ = nullptr;
    size_t off_ = 0;
};

// A helper stream beside caller stream ``s``: helper_fork takes one from the
// pool (idle, or last used by ``s``) and makes it wait for the work queued on
// ``s`` so far; *h = nullptr when ``s`` belongs to another device than the
// current one (run everything on ``s`` then).  helper_join makes ``s`` wait
// for the helper's work and gives the helper back.  0 or TG_EHIP.
int helper_fork(hipStream_t s, hipStream_t* h);
int helper_join(hipStream_t h, hipStream_t s);
void helper_totals(uint64_t* streams, uint64_t* busy);

// Compute units of the current device (grid size of the persistent kernels),
// looked up once per device.
inline int device_cus() {
    // one entry per device, filled by whichever thread gets there first;
    // every thread would store the same value, but the entries are atomics so
    // concurrent tg_seal / tg_open calls on one handle are race-free
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (!v) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            cus <= 0)
            cus = 256;
        cache[dev].store(cus, std::memory_order_relaxed);
        v = cus;
    }
    return v;
}

}  // namespace tg
