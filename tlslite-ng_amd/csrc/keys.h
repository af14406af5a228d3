// keys.h -- key objects (keys.hip): the handle behind tg_key, its pool of
// staging slots for the per-record calls, and the key table's device layout.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "common.h"

// Staging of one per-record call in flight: a mapped pinned buffer, its
// device twin (option stage_copy) and a stream.  A key keeps a pool of them:
// a call takes a free slot (or makes one) and gives it back, so calls on
// copies of one AEAD object (copy.copy shares the handle, recordlayer.py:262,
// :913) from several threads never share a buffer -- ctypes releases the GIL
// around every call.
struct Stage {
    uint8_t* h = nullptr;
    uint8_t* d = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
};

struct tg_key {
    int alg;
    size_t keylen;
    size_t nkeys;
    int device;
    int rounds;
    int taglen;             // 16, or 8 for AES-CCM_8
    void* dev_key;          // GcmKeyDev / GcmTableKey[nkeys] (AES-GCM),
                            // AesKeyDev[nkeys] (AES-CCM), ChachaKeyDev[nkeys]
    std::mutex stage_mu;    // guards the two lists
    std::vector<Stage*> stages;        // every slot of this key
    std::vector<Stage*> free_stages;   // the idle ones (never trimmed before destroy)
};

namespace tg {

inline bool is_ccm(int alg) { return alg == TG_AES_CCM || alg == TG_AES_CCM_8; }

// Makes the key's device the current one.
int select_device(const tg_key* k);

// A free staging slot of this key (a new one if all are in use).  Returns
// TG_OK with *out set, or the error code recorded by fail() (TG_ENOMEM for
// host memory, TG_EHIP when the stream cannot be created).
int take_stage(tg_key* k, Stage** out);
void give_stage(tg_key* k, Stage* st);
// Grows the slot's buffers to at least ``bytes``.
int ensure_stage(Stage* st, size_t bytes);

// A multi-key AES-GCM allocation: GcmTableKey[nkeys], then the 64 GHASH
// powers of each key (gcm_table_wave_kernel, gcm_kt_kernel), then the 15 x 32
// bitsliced key-plane words of each key, MixColumns-folded, in the hybrid
// kernel's row layout (gcm_kt_kernel, kt_planes_kernel), then 16 rotated
// round-key words x 4 per key (gcm_kth_kernel's T-table waves, kt_rot_kernel).
constexpr size_t kTableHpowBytes = 64 * sizeof(uint4);
constexpr size_t kTablePlaneBytes = 15 * 32 * sizeof(uint32_t);
constexpr size_t kTableRotBytes = 16 * sizeof(uint4);
inline uint4* table_hpow(const tg_key* k) {
    return reinterpret_cast<uint4*>(static_cast<uint8_t*>(k->dev_key) + sizeof(GcmTableKey) * k->nkeys);
}
inline uint32_t* table_planes(const tg_key* k) {
    return reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(table_hpow(k)) + kTableHpowBytes * k->nkeys);
}
inline uint4* table_rot(const tg_key* k) {
    return reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(table_planes(k)) + kTablePlaneBytes * k->nkeys);
}

// tg_key_create / tg_key_create_device / tg_key_destroy behind their
// argument checks.
int key_create(int alg, const uint8_t* keys, size_t keylen, size_t nkeys, tg_key** out);
int key_create_device(int alg, const uint8_t* keys, size_t keylen, size_t nkeys, tg_key** out, hipStream_t st);
void key_destroy(tg_key* k);
// tg_key_replace_device / tg_sessions_rekey behind their argument checks:
// entries of the live allocation rebuilt by kernels on ``st`` alone.
int key_replace_device(tg_key* k, const uint32_t* slot, const uint8_t* keys, uint64_t n, hipStream_t st);
int sessions_rekey(tg_key* k, const tg_rekey& r, hipStream_t st);

}  // namespace tg
