// sessions.hip -- counter-mode sequence numbers of a many-session record
// batch (tg_seal_session_records / tg_open_session_records with seq_next).
//
// Every RecordLayer numbers its records in the order it sends them
// (recordlayer.py:522-534 getSeqNumBytes).  A batch that interleaves the
// pending records of many sessions needs, for record i of session s, the
// session's counter plus the count of records of s in front of i: a stable
// per-session rank.  An atomic increment per record would hand the numbers
// out in whatever order the lanes run; this pass is deterministic:
//   1. key[i] = session[i], or nsessions for an index out of range
//   2. stable sort of (key, i) pairs, rocPRIM's merge sort (a block sort,
//      then log2(n / block) merge levels) at every batch size: a session's
//      records become one run, still in batch order.  rocPRIM's radix sort
//      would run the same merge sort up to 2^20 items and Onesweep above,
//      whose kernels carry a private segment; calling merge_sort keeps one
//      algorithm, and no kernel with a private segment, for every n
//   3. max-scan of "position if the run starts here, else 0": every sorted
//      position learns its run's start
//   4. seq[i] = seq_next[key] + (position - run start)
//   5. the last record of each run advances seq_next[key] by the run length
// Step 5 is a launch of its own behind step 4 on the stream, so every read of
// the old counter comes before the first write.  All of it is ordered on the
// caller's stream; temporaries come from the caller's scratch.
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "common.h"

namespace tg {
namespace {

constexpr int kRankThreads = 256;

size_t ru256(size_t v) { return (v + 255) & ~(size_t)255; }

__global__ void rank_keys(const uint32_t* __restrict__ session, uint32_t n, uint64_t nsessions,
                          uint32_t* __restrict__ key) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = session[i];
    key[i] = s < nsessions ? s : (uint32_t)nsessions;   // s >= nsessions: nsessions fits 32 bits
}

// Position p if a run of equal keys starts there, else 0 (the scan's input).
struct RunHead {
    const uint32_t* key;
    __device__ uint32_t operator()(uint32_t p) const { return (p == 0 || key[p] != key[p - 1]) ? p : 0u; }
};

__global__ void rank_scatter(const uint32_t* __restrict__ key, const uint32_t* __restrict__ order,
                             const uint32_t* __restrict__ start, uint32_t n, uint64_t nsessions,
                             const uint64_t* __restrict__ seq_next, uint64_t* __restrict__ seq) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = key[p];
    if (k >= nsessions) return;   // out of range: no number
    seq[order[p]] = seq_next[k] + (uint64_t)(p - start[p]);
}

__global__ void rank_advance(const uint32_t* __restrict__ key, const uint32_t* __restrict__ start, uint32_t n,
                             uint64_t nsessions, uint64_t* __restrict__ seq_next) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = key[p];
    if (k >= nsessions || (p + 1 < n && key[p + 1] == k)) return;   // only a run's last record
    seq_next[k] += (uint64_t)(p - start[p]) + 1u;
}

}  // namespace
}  // namespace tg

// Scratch layout: keys | sorted keys | order | run starts (n u32 each) |
// rocPRIM temporary storage.
int tg_session_rank(const uint32_t* session, uint64_t n, uint64_t nsessions, uint64_t* seq_next,
                    uint64_t* seq, void* scratch, size_t* bytes, hipStream_t s) {
    using namespace tg;
    if (n == 0 || n > 0xffffffffull || nsessions == 0) return TG_EINVAL;
    rocprim::counting_iterator<uint32_t> iota(0);
    size_t t_sort = 0, t_scan = 0;
    auto heads = rocprim::make_transform_iterator(iota, RunHead{nullptr});
    if (rocprim::merge_sort(nullptr, t_sort, (uint32_t*)nullptr, (uint32_t*)nullptr, iota,
                            (uint32_t*)nullptr, (size_t)n, rocprim::less<uint32_t>(), s) != hipSuccess ||
        rocprim::inclusive_scan(nullptr, t_scan, heads, (uint32_t*)nullptr, (size_t)n,
                                rocprim::maximum<uint32_t>(), s) != hipSuccess)
        return TG_EHIP;
    const size_t b32 = ru256(n * 4), tmp = ru256(t_sort > t_scan ? t_sort : t_scan);
    const size_t need = 4 * b32 + tmp;
    if (!scratch) {
        *bytes = need;
        return TG_OK;
    }
    if (*bytes < need || !session || !seq_next || !seq) return TG_EINVAL;
    uint8_t* p = static_cast<uint8_t*>(scratch);
    uint32_t* key = reinterpret_cast<uint32_t*>(p);
    uint32_t* key_sorted = reinterpret_cast<uint32_t*>(p + b32);
    uint32_t* order = reinterpret_cast<uint32_t*>(p + 2 * b32);
    uint32_t* start = reinterpret_cast<uint32_t*>(p + 3 * b32);
    void* t = p + 4 * b32;
    const unsigned blocks = (unsigned)((n + kRankThreads - 1) / kRankThreads);
    hipLaunchKernelGGL(rank_keys, dim3(blocks), dim3(kRankThreads), 0, s, session, (uint32_t)n, nsessions, key);
    size_t ts = t_sort;
    if (rocprim::merge_sort(t, ts, key, key_sorted, iota, order, (size_t)n, rocprim::less<uint32_t>(), s) !=
        hipSuccess)
        return TG_EHIP;
    ts = t_scan;
    if (rocprim::inclusive_scan(t, ts, rocprim::make_transform_iterator(iota, RunHead{key_sorted}), start,
                                (size_t)n, rocprim::maximum<uint32_t>(), s) != hipSuccess)
        return TG_EHIP;
    hipLaunchKernelGGL(rank_scatter, dim3(blocks), dim3(kRankThreads), 0, s, key_sorted, order, start,
                       (uint32_t)n, nsessions, seq_next, seq);
    hipLaunchKernelGGL(rank_advance, dim3(blocks), dim3(kRankThreads), 0, s, key_sorted, start, (uint32_t)n,
                       nsessions, seq_next);
    return hipGetLastError() == hipSuccess ? TG_OK : TG_EHIP;
}
