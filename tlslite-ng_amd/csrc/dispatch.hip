// dispatch.hip -- kernel-selection policy: which launcher a batch takes, by
// algorithm, key count, batch size, record lengths and options.  Every
// measured threshold of that choice lives here.
#include "dispatch.h"

#include "api.h"
#include "common.h"
#include "keys.h"
#include "options.h"
#include "runtime.h"

namespace tg {
namespace {

// Batches that run a lane-per-record kernel (more records than the
// wave-per-record kernels take) with per-record lengths run longest first
// (planner.hip): a wave then holds records of nearly one length instead of
// idling behind its longest.
constexpr uint64_t kPlanMinRecords = 2049;

// Key-table AES-GCM: records of at least this many bytes take the
// key-grouped octet kernel, shorter ones the lane kernel (option kt_split).
constexpr uint32_t kKtSplitDefault = 2048;
// With the short records inside the key-table hybrid (its lane loop runs
// beside the long jobs instead of after them) the split moves down.  With two
// pairs per planned job: config 4 674-676 GiB/s at 1 024 against 663-668 at
// 2 048 (profiles/r06/s2/); with four (TG_KTH_GROUP): 694.5-696.7 at 1 536,
// 694.3-694.6 at 1 280, 693.1-693.8 at 1 792, 690.4 at 2 048, 688.4-689.1 at
// 1 024, 681 at 768 (profiles/r06/s4/, s5/).
constexpr uint32_t kKtSplitFused = 1536;
// Small key-table batches -- at most this many records, or one length with
// at most this many bytes in all -- run one record per wavefront (the wave
// kernel, table-free GHASH, no plan): 0.014 / 0.023 / 0.099 ms for 1 / 2 048 /
// 16 384 records of 1 KiB against 0.23 / 0.32 / 0.34 ms planned, and 0.11
// against 0.21 ms for 2 048 records of 16 KiB (profiles/r04/r4w/).
constexpr uint64_t kKtWaveMaxRecords = 2048;
constexpr uint64_t kKtWaveMaxBytes = 16ull << 20;

int launch_kernels(tg_key* k, const tg_batch& b, bool open, hipStream_t s, const uint32_t* order) {
    if (k->alg == TG_AES_GCM)
        return tg_launch_gcm(static_cast<const GcmKeyDev*>(k->dev_key), k->rounds, b, open, s, order);
    return tg_launch_chacha(static_cast<const ChachaKeyDev*>(k->dev_key), k->nkeys, b, open, s, order);
}

// Key-table AES-GCM (option gcm_table_variant): 0 = auto (small batches one
// record per wavefront, see kKtWaveMaxRecords; otherwise a length split at
// kt_split: the long records on the kernel kt_lpr picks -- 0 = default,
// 8 / 16 / 32 / 64 lanes per record on the key-grouped bitsliced kernel, -1
// the wave-per-record T-table kernel with 4-bit GHASH tables -- the rest on
// the lane kernel, one plan); 1 = the lane kernel for every record; 5 = the
// wave-per-record kernel, table-free GHASH, no plan; 6 = the wave-per-record
// kernel with 4-bit tables for every record; 14 = the octet kernel (8 lanes
// per record) for every record.
constexpr int kKtLprDefault = 32;

int launch_gcm_table(tg_key* k, const tg_batch& b, bool open, hipStream_t s) {
    const auto* keys = static_cast<const GcmTableKey*>(k->dev_key);
    uint32_t split;
    const int o = opt(kOptKtLpr);
    int lpr = o == 0 ? kKtLprDefault : o < 0 ? 0 : o;
    switch (opt(kOptGcmTableVariant)) {
        case 0: {
            const int sp = opt(kOptKtSplit);
            split = sp > 0 ? (uint32_t)sp
                  : lpr == 32 && opt(kOptKtHybrid) >= 0 ? kKtSplitFused : kKtSplitDefault;
            // small batches (unless the split or the long-record kernel is forced)
            if (sp == 0 && o == 0 &&
                (b.n <= kKtWaveMaxRecords || (!b.len && b.n * (uint64_t)b.fixed_len <= kKtWaveMaxBytes)))
                return tg_launch_gcm_table_wave(keys, k->nkeys, table_hpow(k), k->rounds, b, open, s, false);
            break;
        }
        case 1: split = 0xffffffffu; break;
        case 5: return tg_launch_gcm_table_wave(keys, k->nkeys, table_hpow(k), k->rounds, b, open, s, false);
        case 6: split = 0; lpr = 0; break;
        case 14: split = 0; lpr = 8; break;
        default: return TG_EINVAL;
    }
    // One length for every record, below the split (or option no_plan): every
    // record is the lane kernel's and a length order is moot, so no plan --
    // its sort, scans and stream-ordered allocation are pure latency for small
    // multi-session batches (profiles/r04/r4w/).
    if (split != 0 && ((!b.len && b.fixed_len < split) || opt(kOptNoPlan)))
        return tg_launch_gcm_table_lane(keys, k->nkeys, k->rounds, b, open, s, nullptr, nullptr);
    // the long records (lpr 32) on the T-table + bitsliced kernel unless
    // kt_hybrid = -1 (the bitsliced-only key-grouped kernel)
    const bool hybrid = lpr == 32 && opt(kOptKtHybrid) >= 0;
    return tg_launch_gcm_kt(keys, k->nkeys, table_hpow(k), table_planes(k), table_rot(k), k->rounds, b, open, s,
                            split, lpr, hybrid);
}

}  // namespace

// The order and the sort's scratch come from the per-launch scratch cache
// (runtime.h Scratch), so batches in flight on other streams never share
// them.
int launch(tg_key* k, const tg_batch& b, bool open, hipStream_t s) {
    if (is_ccm(k->alg))
        return tg_launch_ccm(static_cast<const AesKeyDev*>(k->dev_key), k->nkeys, k->rounds, k->taglen,
                             b, open, s);
    if (k->alg == TG_AES_GCM && k->nkeys > 1) return launch_gcm_table(k, b, open, s);
    // (ChaCha key tables take the wave kernel too: chacha_wave_kernel<.., MULTIKEY>)
    const bool wave = (k->nkeys == 1 && k->alg == TG_AES_GCM && tg_gcm_wave_path(b.n)) ||
                      (k->alg == TG_CHACHA20_POLY1305 && tg_chacha_wave_path(b.n));
    if (!b.len || b.n < kPlanMinRecords || wave || b.n > 0xffffffffull || opt(kOptNoPlan))
        return launch_kernels(k, b, open, s, nullptr);
    size_t sort = 0;
    int rc = tg_length_order(b.len, b.n, nullptr, nullptr, &sort, s);
    if (rc) return rc;
    Scratch scratch(s);
    if (scratch.alloc(align_up(b.n * sizeof(uint32_t), 256) + sort)) return fail(TG_EHIP, "scratch allocation failed");
    uint32_t* order = scratch.take<uint32_t>(b.n * sizeof(uint32_t), 256);
    rc = tg_length_order(b.len, b.n, order, scratch.take<uint8_t>(sort, 256), &sort, s);
    if (!rc) rc = launch_kernels(k, b, open, s, order);
    if (scratch.release() && !rc) rc = TG_EHIP;
    return rc;
}

}  // namespace tg
