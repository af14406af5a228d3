// aead.hip -- the AEAD calls behind the ABI: the per-record drop-in path that
// the ctypes objects behind tlsgpu.cipherfactory call for every record
// (recordlayer.py:558, :821), through a staging slot of the key, and the
// device-pointer batch entry.
#include <cstring>

#include "api.h"
#include "common.h"
#include "dispatch.h"
#include "keys.h"
#include "options.h"

namespace tg {
namespace {

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// The record's round trip through one staging slot (single()).
int single_staged(tg_key* k, Stage* st, const uint8_t* nonce, const uint8_t* aad, size_t aadlen,
                  const uint8_t* in, size_t inlen, uint8_t* out, bool open, size_t len, size_t outlen,
                  size_t o_aad, size_t o_in, size_t o_out, size_t o_st, size_t total) {
    int rc = ensure_stage(st, total);
    if (rc) return rc;
    memcpy(st->h, nonce, 12);
    if (aadlen) memcpy(st->h + o_aad, aad, aadlen);
    if (inlen) memcpy(st->h + o_in, in, inlen);
    // Zero copy by default: the kernel reads and writes the mapped pinned
    // staging buffer over PCIe, so a record costs one launch and one
    // synchronisation instead of two copies more (option stage_copy: copy
    // through device memory instead).
    const bool copy = opt(kOptStageCopy) != 0;
    uint8_t* base = st->d;
    if (!copy) {
        void* dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, st->h, 0));
        base = static_cast<uint8_t*>(dp);
    } else {
        HIP_TRY(hipMemcpyAsync(st->d, st->h, o_out, hipMemcpyHostToDevice, st->stream));
    }
    tg_batch b;
    memset(&b, 0, sizeof(b));
    b.n = 1;
    b.in = base + o_in;
    b.fixed_len = (uint32_t)len;
    b.fixed_aad_len = (uint32_t)aadlen;
    b.out = base + o_out;
    b.nonce = base;
    b.aad = base + o_aad;
    b.status = open ? base + o_st : nullptr;
    if ((rc = launch(k, b, open, st->stream))) return fail(rc, "kernel launch failed");
    if (copy)
        HIP_TRY(hipMemcpyAsync(st->h + o_out, st->d + o_out, total - o_out, hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    if (open) {
        const int ok = st->h[o_st] == 1;
        if (ok && len) memcpy(out, st->h + o_out, len);
        if (!ok && len) memset(out, 0, len);
        return ok;
    }
    memcpy(out, st->h + o_out, outlen);
    return TG_OK;
}

}  // namespace

// One record through the staging buffers: [nonce | aad | input | output | status]
int single(tg_key* k, const uint8_t* nonce, size_t noncelen, const uint8_t* aad, size_t aadlen,
           const uint8_t* in, size_t inlen, uint8_t* out, bool open) {
    if (!k) return fail(TG_EINVAL, "null key");
    if (k->nkeys != 1) return fail(TG_EINVAL, "per-record calls need a single-key handle");
    if (noncelen != 12) return fail(TG_ENONCE, "Bad nonce length");
    if ((aadlen && !aad) || (inlen && !in)) return fail(TG_EINVAL, "null buffer");
    const size_t T = (size_t)k->taglen;
    if (open && inlen < T) {   // aesgcm.py:135-136, chacha20_poly1305.py:76-77, aesccm.py:120-123
        return 0;
    }
    const size_t len = open ? inlen - T : inlen;
    if (len > 0xffffffffull || aadlen > 0xffffffffull) return fail(TG_EINVAL, "record too long");
    if (is_ccm(k->alg) && len >= (1ull << 28) - 32) return fail(TG_EINVAL, "CCM record too long");
    const size_t o_aad = 16, o_in = align16(o_aad + aadlen), o_out = align16(o_in + inlen);
    const size_t outlen = open ? len : len + T;
    const size_t o_st = align16(o_out + outlen), total = o_st + 16;
    int rc = select_device(k);
    if (rc) return rc;
    Stage* st = nullptr;
    if ((rc = take_stage(k, &st))) return rc;
    rc = single_staged(k, st, nonce, aad, aadlen, in, inlen, out, open, len, outlen, o_aad, o_in, o_out,
                       o_st, total);
    give_stage(k, st);
    return rc;
}

int batch(tg_key* k, const tg_batch* b, void* stream, bool open) {
    if (!k || !b) return fail(TG_EINVAL, "null argument");
    if (b->n == 0) return TG_OK;
    if (!b->in || !b->out || !b->nonce) return fail(TG_EINVAL, "null device buffer");
    if (!b->aad && (b->aad_len || b->fixed_aad_len)) return fail(TG_EINVAL, "null aad");
    if (k->nkeys > 1 && !b->key_idx) return fail(TG_EINVAL, "key table needs key_idx");
    if (k->nkeys == 1 && b->key_idx) return fail(TG_EINVAL, "key_idx given for a single key");
    int rc = select_device(k);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream
    if ((rc = launch(k, *b, open, s))) return fail(rc, "kernel launch failed: %s",
                                                   hipGetErrorString(hipGetLastError()));
    if (open && k->nkeys > 1 && (rc = tg_launch_zero_skipped(*b, k->nkeys, s)))
        return fail(rc, "zeroing skipped records failed");
    return TG_OK;
}

}  // namespace tg
