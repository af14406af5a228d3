// api.hip -- the C ABI of libtlsgpu.so (declared in include/tlsgpu.h): the
// entry points with their argument checks and the error text.  What they do
// is in keys.hip (key objects), aead.hip (per-record and batch calls),
// framing.hip (record framing), dispatch.hip (kernel selection) and
// runtime.hip (scratch and helper streams).  No exceptions cross the ABI.
#include "api.h"

#include <cstdarg>
#include <cstdio>
#include <string>

#include "common.h"
#include "host.h"
#include "keys.h"
#include "options.h"
#include "runtime.h"

namespace {

thread_local std::string g_err;

// tg_version()'s text; a measurement build appends its flags (common.h).
std::string& version_text() {
    static std::string v = "tlsgpu 0.1.0 (gfx950)";
    return v;
}

}  // namespace

namespace tg {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

void note_measurement_build(const char* flag) {
    std::string& v = version_text();
    if (v.find("MEASUREMENT BUILD") == std::string::npos) v += " MEASUREMENT BUILD (not the product):";
    v += " ";
    v += flag;
}

}  // namespace tg

using tg::fail;

extern "C" {

const char* tg_version(void) { return version_text().c_str(); }

const char* tg_last_error(void) { return g_err.c_str(); }

int tg_device_count(int* count) {
    if (!count) return fail(TG_EINVAL, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(TG_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return TG_OK;
}

int tg_set_option(const char* name, int value) {
    const int o = tg::opt_index(name);
    if (o < 0) return fail(TG_EINVAL, "unknown option %s", name ? name : "(null)");
    tg::opt_set(static_cast<tg::Opt>(o), value);
    return TG_OK;
}

int tg_get_option(const char* name, int* value) {
    const int o = tg::opt_index(name);
    if (o < 0 || !value) return fail(TG_EINVAL, "unknown option %s", name ? name : "(null)");
    *value = tg::opt(static_cast<tg::Opt>(o));
    return TG_OK;
}

int tg_init(int device) {
    int n = 0;
    int rc = tg_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n) return fail(TG_ENODEV, "device %d not present (%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    return TG_OK;
}

int tg_key_create(int alg, const uint8_t* keys, size_t keylen, size_t nkeys, tg_key** out) {
    if (!out || !keys || nkeys == 0) return fail(TG_EINVAL, "null argument");
    return tg::key_create(alg, keys, keylen, nkeys, out);
}

int tg_key_create_device(int alg, const uint8_t* keys, size_t keylen, size_t nkeys,
                         tg_key** out, void* stream) {
    if (!out || !keys || nkeys == 0) return fail(TG_EINVAL, "null argument");
    return tg::key_create_device(alg, keys, keylen, nkeys, out, static_cast<hipStream_t>(stream));
}

int tg_hkdf_expand_label(int hashlen, const uint8_t* secrets, uint64_t n, const uint8_t* label,
                         size_t labellen, const uint8_t* context, size_t ctxlen, size_t outlen,
                         uint8_t* out, void* stream) {
    if (hashlen != 32 && hashlen != 48) return fail(TG_EINVAL, "hash length must be 32 or 48");
    if (outlen == 0 || outlen > (size_t)hashlen)
        return fail(TG_EINVAL, "output length must be 1..%d", hashlen);
    if ((labellen && !label) || (ctxlen && !context)) return fail(TG_EINVAL, "null label");
    if (n == 0) return TG_OK;
    if (!secrets || !out) return fail(TG_EINVAL, "null device buffer");
    tg::HkdfMsg msg;
    if (tg::host::hkdf_message(hashlen, label, labellen, context, ctxlen, outlen, &msg))
        return fail(TG_EINVAL, "label or context too long");
    int rc = tg_launch_hkdf(hashlen, msg, secrets, n, out, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "hkdf launch failed") : TG_OK;
}

int tg_key_replace_device(tg_key* k, const uint32_t* slot, const uint8_t* keys, uint64_t n, void* stream) {
    if (!keys && n) return fail(TG_EINVAL, "null keys");   // no rows, nothing to point at
    if (!k) return fail(TG_EINVAL, "null key");
    if (n > k->nkeys)
        return fail(TG_EINVAL, "n (%llu) is above the key handle's nkeys (%llu)", (unsigned long long)n,
                    (unsigned long long)k->nkeys);
    if (n == 0) return TG_OK;
    return tg::key_replace_device(k, slot, keys, n, static_cast<hipStream_t>(stream));
}

// Argument errors come first, before any HIP call; those of the struct alone
// are reported whatever the key is.
int tg_sessions_rekey(tg_key* k, const tg_rekey* r, void* stream) {
    if (!r) return fail(TG_EINVAL, "null tg_rekey");
    if (r->mode != TG_REKEY_INSTALL && r->mode != TG_REKEY_UPDATE)
        return fail(TG_EINVAL, "mode %u is neither TG_REKEY_INSTALL nor TG_REKEY_UPDATE", r->mode);
    if (r->hashlen != 32 && r->hashlen != 48) return fail(TG_EINVAL, "hashlen must be 32 or 48, got %u", r->hashlen);
    if (!r->iv_table) return fail(TG_EINVAL, "null iv_table");
    if (r->mode == TG_REKEY_UPDATE && !r->secrets)
        return fail(TG_EINVAL, "TG_REKEY_UPDATE needs the secrets table");
    if (r->mode == TG_REKEY_UPDATE && r->new_secrets)
        return fail(TG_EINVAL, "TG_REKEY_UPDATE takes no new_secrets");
    if (r->mode == TG_REKEY_INSTALL && !r->new_secrets) return fail(TG_EINVAL, "TG_REKEY_INSTALL needs new_secrets");
    if (!k) return fail(TG_EINVAL, "null key");
    if (r->nsessions != k->nkeys)
        return fail(TG_EINVAL, "nsessions (%llu) must equal the key handle's nkeys (%llu)",
                    (unsigned long long)r->nsessions, (unsigned long long)k->nkeys);
    if (r->n > k->nkeys)
        return fail(TG_EINVAL, "n (%llu) is above the key handle's nkeys (%llu)", (unsigned long long)r->n,
                    (unsigned long long)k->nkeys);
    if (r->n == 0) return TG_OK;
    return tg::sessions_rekey(k, *r, static_cast<hipStream_t>(stream));
}

int tg_key_destroy(tg_key* k) {
    if (k) tg::key_destroy(k);
    return TG_OK;
}

int tg_key_info(const tg_key* k, int* alg, size_t* keylen, size_t* nkeys) {
    if (!k) return fail(TG_EINVAL, "null key");
    if (alg) *alg = k->alg;
    if (keylen) *keylen = k->keylen;
    if (nkeys) *nkeys = k->nkeys;
    return TG_OK;
}

int tg_key_taglen(const tg_key* k) {
    if (!k) return fail(TG_EINVAL, "null key");
    return k->taglen;
}

int tg_seal(tg_key* k, const uint8_t* nonce, size_t noncelen, const uint8_t* aad, size_t aadlen,
            const uint8_t* pt, size_t len, uint8_t* out) {
    if (!out) return fail(TG_EINVAL, "null output");
    return tg::single(k, nonce, noncelen, aad, aadlen, pt, len, out, false);
}

int tg_open(tg_key* k, const uint8_t* nonce, size_t noncelen, const uint8_t* aad, size_t aadlen,
            const uint8_t* in, size_t inlen, uint8_t* pt) {
    if (!pt && k && inlen > (size_t)k->taglen) return fail(TG_EINVAL, "null output");
    return tg::single(k, nonce, noncelen, aad, aadlen, in, inlen, pt, true);
}

int tg_seal_batch(tg_key* k, const tg_batch* b, void* stream) { return tg::batch(k, b, stream, false); }

int tg_open_batch(tg_key* k, const tg_batch* b, void* stream) { return tg::batch(k, b, stream, true); }

int tg_seal_records(tg_key* k, const tg_records* r, void* stream) { return tg::records(k, r, stream, true); }

int tg_open_records(tg_key* k, const tg_records* r, void* stream) { return tg::records(k, r, stream, false); }

int tg_seal_session_records(tg_key* k, const tg_session_records* r, void* stream) {
    return tg::session_records(k, r, stream, true);
}

int tg_open_session_records(tg_key* k, const tg_session_records* r, void* stream) {
    return tg::session_records(k, r, stream, false);
}

int tg_make_nonces(int mode, const uint8_t* iv, size_t ivlen, uint64_t seq0, uint64_t n,
                   uint8_t* out, void* stream) {
    if (!iv || !out) return fail(TG_EINVAL, "null argument");
    if (!((mode == 0 && ivlen == 12) || (mode == 1 && ivlen == 4)))
        return fail(TG_EINVAL, "mode %d needs a %d-byte iv", mode, mode == 0 ? 12 : 4);
    if (n == 0) return TG_OK;
    int rc = tg_launch_nonces(mode, iv, seq0, n, out, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "nonce kernel launch failed") : TG_OK;
}

int tg_malloc(void** p, size_t bytes) {
    if (!p) return fail(TG_EINVAL, "null argument");
    HIP_TRY(hipMalloc(p, bytes ? bytes : 1));
    return TG_OK;
}

int tg_free(void* p) {
    if (p) HIP_TRY(hipFree(p));
    return TG_OK;
}

int tg_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
    if (!bytes) return TG_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return TG_OK;
}

int tg_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
    if (!bytes) return TG_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return TG_OK;
}

int64_t tg_scan_records(const uint8_t* buf, size_t len, uint32_t max_body, uint64_t* off,
                        uint32_t* rlen, size_t max_n, size_t* consumed) {
    if (!consumed || (len && !buf) || (max_n && (!off || !rlen)))
        return fail(TG_EINVAL, "null argument");
    tg::host::ScanError err{};
    const int64_t k = tg::host::scan_records(buf, len, max_body, off, rlen, max_n, consumed, &err);
    if (k >= 0) return k;
    if (err.code == 1) return fail(TG_EHEADER, "record %zu: content type %u", err.index, err.value);
    return fail(TG_EOVERFLOW, "record %zu: %u > %u bytes", err.index, err.value, max_body);
}

int tg_gather(const uint8_t* src, const uint64_t* src_off, const uint32_t* len, uint8_t* dst,
              const uint64_t* dst_off, uint64_t n, void* stream) {
    if (n && (!src || !src_off || !len || !dst || !dst_off)) return fail(TG_EINVAL, "null argument");
    if (n == 0) return TG_OK;
    int rc = tg_launch_gather(src, src_off, len, dst, dst_off, n, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "gather kernel launch failed") : TG_OK;
}

int tg_host_copy(void* dst, const void* src, size_t bytes, int nthreads) {
    if (bytes && (!dst || !src)) return fail(TG_EINVAL, "null buffer");
    tg::host::parallel_copy(dst, src, bytes, nthreads);
    return TG_OK;
}

int tg_host_copy_rows(void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t row_bytes,
                      size_t rows, int nthreads) {
    if (rows && row_bytes && (!dst || !src)) return fail(TG_EINVAL, "null buffer");
    if (rows > 1 && (dst_stride < row_bytes || src_stride < row_bytes)) return fail(TG_EINVAL, "stride below row");
    tg::host::parallel_copy_rows(static_cast<uint8_t*>(dst), dst_stride, static_cast<const uint8_t*>(src),
                                 src_stride, row_bytes, rows, nthreads);
    return TG_OK;
}

int tg_scratch_info(uint64_t* bytes, uint64_t* buffers) {
    if (!bytes || !buffers) return fail(TG_EINVAL, "null argument");
    tg::scratch_totals(bytes, buffers);
    return TG_OK;
}

int tg_scratch_trim(uint64_t keep_bytes) {
    tg::scratch_trim((size_t)keep_bytes);
    return TG_OK;
}

int tg_helper_info(uint64_t* streams, uint64_t* busy) {
    if (!streams || !busy) return fail(TG_EINVAL, "null argument");
    tg::helper_totals(streams, busy);
    return TG_OK;
}

int tg_stream_sync(void* stream) {
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return TG_OK;
}

}  // extern "C"
