// keys.hip -- key objects (keys.h): AES key schedule and GHASH tables built
// once per key, like AESGCM.__init__ at tlslite/utils/aesgcm.py:27-57, from
// host bytes (tg_key_create) or device bytes (tg_key_create_device), and the
// staging slots a key lends to the per-record calls.
#include "keys.h"

#include <cstddef>
#include <cstring>
#include <new>

#include "api.h"
#include "host.h"

namespace tg {
namespace {

// host.cpp fills the GcmKeyDev image without HIP types: same layout.
#define TG_SAME_OFFSET(m) static_assert(offsetof(GcmKeyDev, m) == offsetof(host::GcmKeyImage, m), #m)
static_assert(sizeof(GcmKeyDev) == sizeof(host::GcmKeyImage), "GcmKeyDev image size");
TG_SAME_OFFSET(rounds);
TG_SAME_OFFSET(ghash);
TG_SAME_OFFSET(hpow);
TG_SAME_OFFSET(ghash64);
TG_SAME_OFFSET(ghash8);
TG_SAME_OFFSET(bs8mask);
TG_SAME_OFFSET(bs8rows);
TG_SAME_OFFSET(rkrot);
#undef TG_SAME_OFFSET

void free_stage(Stage* st) {
    if (st->h) (void)hipHostFree(st->h);
    if (st->d) (void)hipFree(st->d);
    if (st->stream) (void)hipStreamDestroy(st->stream);
    delete st;
}

// The table's derived arrays on the device: H^1..H^64 and the key planes.
int table_derive(tg_key* k, hipStream_t s) {
    const auto* keys = static_cast<const GcmTableKey*>(k->dev_key);
    int rc = tg_launch_table_hpow(keys, k->nkeys, table_hpow(k), s);
    if (!rc) rc = tg_launch_kt_planes(keys, k->nkeys, k->rounds, table_planes(k), table_rot(k), s);
    return rc;
}

size_t dev_key_bytes(const tg_key* k) {
    if (k->alg == TG_CHACHA20_POLY1305) return sizeof(ChachaKeyDev) * k->nkeys;
    if (is_ccm(k->alg)) return sizeof(AesKeyDev) * k->nkeys;
    return k->nkeys > 1 ? (sizeof(GcmTableKey) + kTableHpowBytes + kTablePlaneBytes + kTableRotBytes) * k->nkeys
                        : sizeof(GcmKeyDev);
}

// Validate (alg, keylen, nkeys) and allocate a handle with its stream.
int new_key(int alg, size_t keylen, size_t nkeys, tg_key** out) {
    *out = nullptr;
    if (alg == TG_AES_GCM || is_ccm(alg)) {
        // AssertionError in AESGCM.__init__ (aesgcm.py:37-38) and AESCCM.__init__ (aesccm.py:22-30)
        if (keylen != 16 && keylen != 32) return fail(TG_EKEYLEN, "AES key must be 16 or 32 bytes");
    } else if (alg == TG_CHACHA20_POLY1305) {
        if (keylen != 32) return fail(TG_EKEYLEN, "Key must be 256 bit long");
    } else {
        return fail(TG_EINVAL, "unknown algorithm %d", alg);
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    tg_key* k = new (std::nothrow) tg_key();
    if (!k) return fail(TG_ENOMEM, "out of host memory");
    k->alg = alg;
    k->keylen = keylen;
    k->nkeys = nkeys;
    k->taglen = alg == TG_AES_CCM_8 ? 8 : 16;
    k->rounds = alg == TG_CHACHA20_POLY1305 ? 0 : (keylen == 16 ? 10 : 14);
    k->device = dev;
    *out = k;
    return TG_OK;
}

// The key's device allocation, its front filled from a host image of
// ``count`` elements T, each zeroed and then filled by fill(element, index).
// The image is scrubbed before it is freed.
template <class T, class Fill>
int upload(tg_key* k, size_t count, Fill fill) {
    T* hk = new (std::nothrow) T[count];
    if (!hk) return fail(TG_ENOMEM, "out of host memory");
    const size_t bytes = sizeof(T) * count;
    memset(hk, 0, bytes);
    for (size_t i = 0; i < count; ++i) fill(hk[i], i);
    hipError_t e = hipMalloc(&k->dev_key, dev_key_bytes(k));
    if (e == hipSuccess) e = hipMemcpy(k->dev_key, hk, bytes, hipMemcpyHostToDevice);
    memset(hk, 0, bytes);
    delete[] hk;
    return e == hipSuccess ? TG_OK : fail(TG_EHIP, "key upload: %s", hipGetErrorString(e));
}

// A finished key to the caller, or a failed one destroyed.
int hand_over(tg_key* k, int rc, tg_key** out) {
    if (rc) key_destroy(k);
    else *out = k;
    return rc;
}

}  // namespace

int select_device(const tg_key* k) {
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != k->device) HIP_TRY(hipSetDevice(k->device));
    return TG_OK;
}

int take_stage(tg_key* k, Stage** out) {
    {
        std::lock_guard<std::mutex> g(k->stage_mu);
        if (!k->free_stages.empty()) {
            *out = k->free_stages.back();
            k->free_stages.pop_back();
            return TG_OK;
        }
    }
    Stage* st = new (std::nothrow) Stage();
    if (!st) return fail(TG_ENOMEM, "out of host memory");
    hipError_t e = hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete st;
        return fail(TG_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> g(k->stage_mu);
    k->stages.push_back(st);
    *out = st;
    return TG_OK;
}

// A slot given back stays with the key until tg_key_destroy: the pool is as
// large as the most calls the key has had in flight at once, so bursts of
// concurrent calls reuse their slots instead of destroying streams and
// freeing pinned memory (which can synchronise the device) after each burst
// (ADVICE r04).
void give_stage(tg_key* k, Stage* st) {
    std::lock_guard<std::mutex> g(k->stage_mu);
    k->free_stages.push_back(st);
}

int ensure_stage(Stage* st, size_t bytes) {
    if (bytes <= st->cap) return TG_OK;
    size_t cap = st->cap ? st->cap : 65536;
    while (cap < bytes) cap *= 2;
    if (st->h) (void)hipHostFree(st->h);
    if (st->d) (void)hipFree(st->d);
    st->h = nullptr;
    st->d = nullptr;
    st->cap = 0;
    HIP_TRY(hipHostMalloc((void**)&st->h, cap, hipHostMallocMapped));
    HIP_TRY(hipMalloc((void**)&st->d, cap));
    st->cap = cap;
    return TG_OK;
}

int key_create(int alg, const uint8_t* keys, size_t keylen, size_t nkeys, tg_key** out) {
    tg_key* k = nullptr;
    int rc = new_key(alg, keylen, nkeys, &k);
    if (rc) return rc;
    if (is_ccm(alg)) {
        rc = upload<AesKeyDev>(k, nkeys, [&](AesKeyDev& hk, size_t i) {
            k->rounds = host::aes_round_words(keys + keylen * i, keylen, hk.rk, nullptr);
        });
    } else if (alg == TG_AES_GCM && nkeys > 1) {
        rc = upload<GcmTableKey>(k, nkeys, [&](GcmTableKey& hk, size_t i) {
            k->rounds = host::aes_round_words(keys + keylen * i, keylen, hk.rk, hk.hn);
        });
        hipError_t e = hipSuccess;
        if (!rc && table_derive(k, nullptr)) rc = fail(TG_EHIP, "key powers launch failed");
        if (!rc && (e = hipDeviceSynchronize()) != hipSuccess)
            rc = fail(TG_EHIP, "key powers: %s", hipGetErrorString(e));
    } else if (alg == TG_AES_GCM) {
        rc = upload<host::GcmKeyImage>(k, 1, [&](host::GcmKeyImage& hk, size_t) {
            host::gcm_key_image(keys, keylen, &hk);   // key length checked by new_key
            k->rounds = (int)hk.rounds;
        });
    } else {
        rc = upload<ChachaKeyDev>(k, nkeys, [&](ChachaKeyDev& hk, size_t i) {
            for (int w = 0; w < 8; ++w) hk.k[w] = host::le32(keys + 32 * i + 4 * w);
        });
    }
    return hand_over(k, rc, out);
}

int key_create_device(int alg, const uint8_t* keys, size_t keylen, size_t nkeys, tg_key** out, hipStream_t st) {
    tg_key* k = nullptr;
    int rc = new_key(alg, keylen, nkeys, &k);
    if (rc) return rc;
    const size_t bytes = dev_key_bytes(k);
    hipError_t e = hipMalloc(&k->dev_key, bytes);
    if (e != hipSuccess) {
        rc = fail(TG_EHIP, "key alloc: %s", hipGetErrorString(e));
    } else if (alg == TG_CHACHA20_POLY1305) {   // ChachaKeyDev is the raw key bytes (LE words)
        e = hipMemcpyAsync(k->dev_key, keys, 32 * nkeys, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) rc = fail(TG_EHIP, "key copy: %s", hipGetErrorString(e));
    } else {
        const int layout = is_ccm(alg) ? 2 : (nkeys > 1 ? 1 : 0);
        rc = tg_launch_aes_setup((int)keylen, layout, keys, nkeys, k->dev_key, st);
        if (!rc && layout == 1) rc = table_derive(k, st);
        if (rc) rc = fail(rc, "key setup launch failed");
    }
    if (!rc && (e = hipStreamSynchronize(st)) != hipSuccess)
        rc = fail(TG_EHIP, "key setup: %s", hipGetErrorString(e));
    return hand_over(k, rc, out);
}

namespace {

// Entries of a live allocation rebuilt on ``st``: the fused front kernel, then
// (AES-GCM table) the slot forms of the derive kernels over the same list.
// No allocation, no copy to the host and no synchronisation.
int rebuild(tg_key* k, int hashlen, const HkdfMsg* msgs, const uint32_t* slot, const uint8_t* src,
            uint8_t* secrets, uint8_t* iv_table, uint64_t* seq_next, uint64_t n, hipStream_t st) {
    const int layout = k->alg == TG_CHACHA20_POLY1305 ? 3 : is_ccm(k->alg) ? 2 : (k->nkeys > 1 ? 1 : 0);
    int rc = tg_launch_rekey(hashlen, (int)k->keylen, layout, msgs, slot, src, secrets, iv_table, seq_next, n,
                             k->nkeys, k->dev_key, st);
    if (!rc && layout == 1) {
        const auto* keys = static_cast<const GcmTableKey*>(k->dev_key);
        rc = tg_launch_table_hpow(keys, n, table_hpow(k), st, slot, k->nkeys);
        if (!rc) rc = tg_launch_kt_planes(keys, n, k->rounds, table_planes(k), table_rot(k), st, slot, k->nkeys);
    }
    return rc ? fail(rc, "rekey launch failed: %s", hipGetErrorString(hipGetLastError())) : TG_OK;
}

}  // namespace

int key_replace_device(tg_key* k, const uint32_t* slot, const uint8_t* keys, uint64_t n, hipStream_t st) {
    int rc = select_device(k);
    if (rc) return rc;
    return rebuild(k, 0, nullptr, slot, keys, nullptr, nullptr, nullptr, n, st);
}

int sessions_rekey(tg_key* k, const tg_rekey& r, hipStream_t st) {
    HkdfMsg msgs[3];
    const size_t h = r.hashlen;
    if (host::hkdf_message((int)h, (const uint8_t*)"traffic upd", 11, nullptr, 0, h, &msgs[0]) ||
        host::hkdf_message((int)h, (const uint8_t*)"key", 3, nullptr, 0, k->keylen, &msgs[1]) ||
        host::hkdf_message((int)h, (const uint8_t*)"iv", 2, nullptr, 0, 12, &msgs[2]))
        return fail(TG_EINVAL, "label too long");
    int rc = select_device(k);
    if (rc) return rc;
    return rebuild(k, (int)h, msgs, r.slot, r.new_secrets, r.secrets, r.iv_table, r.seq_next, r.n, st);
}

void key_destroy(tg_key* k) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != k->device) (void)hipSetDevice(k->device);
    // Batches may still be running on caller streams (tg_seal_batch and
    // friends take any stream): wait for the whole device before the key
    // material is scrubbed and released, so no launch ever reads a zeroed or
    // freed schedule.
    (void)hipDeviceSynchronize();
    if (k->dev_key) {
        // scrub key material before release
        (void)hipMemset(k->dev_key, 0, dev_key_bytes(k));
        (void)hipFree(k->dev_key);
    }
    for (Stage* st : k->stages) free_stage(st);   // no call may be in flight on k any more
    if (cur >= 0 && cur != k->device) (void)hipSetDevice(cur);
    delete k;
}

}  // namespace tg
