// tls13.hip -- the TLS 1.3 key schedule on the device: from the (EC)DHE shared
// secret, an optional PSK and the transcript hashes to the traffic secrets that
// tg_sessions_rekey installs, with the Finished values on the way
// (tg_hkdf_extract, tg_hkdf_expand_label_rows, tg_tls13_finished,
// tg_tls13_handshake_secrets, tg_tls13_application_secrets).
//
// Restates, one session per lane:
//   secureHMAC (tlslite/utils/cryptomath.py:128-132) as HKDF-Extract:
//     Extract(salt, ikm) = HMAC-Hash(salt, ikm);
//   HKDF_expand_label (:155-173) with one context per session, and
//     derive_secret (:175-195), its case context = a transcript hash,
//     outlen = hash length;
//   the schedule of tlsconnection.py:3036-3050 (early secret, "derived",
//     handshake secret, "c hs traffic" / "s hs traffic"), :3203-3224 and :3326
//     ("derived", master secret, "c ap traffic" / "s ap traffic" / "exp master")
//     and the Finished MAC of :3210-3216 and handshakehelpers.py:44-61.
//
// Layout.  A session's part of a hashed message -- the IKM of an Extract, the
// context of an Expand-Label, the transcript hash of a Finished -- is read by
// its own lane, byte by byte, straight into the message words (hm_row): no
// template in scratch and no packing launch.  The bytes around it are the same
// for every session and come as kernel arguments: the HkdfLabel bytes in front
// of the context as LabelPre, a whole shared message (the "derived" and
// "finished" labels) as the HkdfMsg that hkdf_kernel takes.  Secrets enter as
// the two HMAC midstates (keysetup_dev.h), computed once per lane; every secret
// between a stage's input and its outputs stays in registers.  Every loop's
// trip count and every branch on a message position depend on lengths alone,
// and nothing is held in an array indexed at run time: no kernel here has a
// private segment.
#include "prf_dev.h"

#include <string.h>

namespace tg {
namespace {

// The HkdfLabel bytes in front of the context (length, "tls13 " + label, the
// context's length byte) as big-endian words: 10 + labellen <= 42 bytes.
struct LabelPre {
    uint32_t w[11];
    uint32_t len;
};

// A digest as an HMAC key.
template <class H>
__device__ __forceinline__ void digest_key(const typename H::word st[8], typename H::word key[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) key[k] = k < H::kStateOut ? st[k] : typename H::word(0);
}

// st = HMAC under h of   pre || row[0, len) || (COUNTER ? 0x01 : nothing),
// SHA-padded here: the terminator and the bit length are placed by pre.len and
// len alone.  row NULL: len zero bytes.  Only row[0, len) is read.
template <class H, bool COUNTER>
__device__ __forceinline__ void hm_row(const Hm<H>& h, const LabelPre& pre, const uint8_t* row, uint32_t len,
                                       typename H::word st[8]) {
    using W = typename H::word;
    constexpr int WB = sizeof(W);
    const gptr_c r = (gptr_c)row;
    const uint32_t p = pre.len, end = p + len, fin = end + (COUNTER ? 1u : 0u);   // fin: the 0x80
    const uint32_t nb = (fin + 1 + H::kLenBytes + H::kBlock - 1) / H::kBlock;
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = h.in[k];
    for (uint32_t b = 0; b < nb; ++b) {   // uniform: nb comes from the lengths
        const uint32_t base = b * H::kBlock;
        W blk[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            W v = 0;
#pragma unroll
            for (int j = 0; j < WB; ++j) {
                constexpr int kPreBytes = 4 * 11;
                const int c = k * WB + j;             // compile-time position inside the block
                const uint32_t at = base + (uint32_t)c;
                uint32_t byte = 0;
                if (c < kPreBytes && at < p) {        // p < kPreBytes: block 0 only
                    byte = (pre.w[c < kPreBytes ? c / 4 : 0] >> (8 * (3 - c % 4))) & 0xffu;
                } else if (at < end) {
                    if (row) byte = r[at - p];
                } else if (COUNTER && at == end) {
                    byte = 1;
                } else if (at == fin) {
                    byte = 0x80;
                }
                v = (W)((v << 8) | byte);
            }
            blk[k] = v;
        }
        if (b == nb - 1) blk[15] = (W)((H::kBlock + fin) * 8u);   // the key block comes first
        H::compress(st, blk);
    }
    hm_outer<H>(h, st);
}

// ---- tg_hkdf_extract -------------------------------------------------------------
template <class H>
__global__ __launch_bounds__(256) void tls13_extract_kernel(const uint8_t* __restrict__ salts,
                                                            const uint8_t* __restrict__ ikm, uint32_t ikmlen,
                                                            uint64_t n, uint8_t* __restrict__ out) {
    using W = typename H::word;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    W key[16], st[8];
    key_from_row<H, H::kHash, true>(salts ? salts + (uint64_t)H::kHash * i : nullptr, key);
    Hm<H> h;
    hm_key<H>(key, h);
    const LabelPre none{};
    hm_row<H, false>(h, none, ikm ? ikm + (uint64_t)ikmlen * i : nullptr, ikmlen, st);
    store_digest<H>(st, out + (uint64_t)H::kHash * i);
}

// ---- tg_hkdf_expand_label_rows ---------------------------------------------------
template <class H>
__global__ __launch_bounds__(256) void tls13_expand_rows_kernel(LabelPre pre, const uint8_t* __restrict__ secrets,
                                                                const uint8_t* __restrict__ contexts,
                                                                uint32_t ctxlen, uint64_t n, uint32_t outlen,
                                                                uint8_t* __restrict__ out) {
    using W = typename H::word;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    W key[16], st[8];
    key_from_row<H, H::kHash>(secrets + (uint64_t)H::kHash * i, key);
    Hm<H> h;
    hm_key<H>(key, h);
    hm_row<H, true>(h, pre, contexts ? contexts + (uint64_t)ctxlen * i : nullptr, ctxlen, st);
    store_digest_bytes<H>(st, out + (uint64_t)outlen * i, outlen);
}

// ---- tg_tls13_finished -----------------------------------------------------------
// fin: HkdfLabel("finished", "", hash length); the finished key stays in registers.
template <class H>
__global__ __launch_bounds__(256) void tls13_finished_kernel(tg::HkdfMsg fin, const uint8_t* __restrict__ secrets,
                                                             const uint8_t* __restrict__ hashes, uint64_t n,
                                                             uint8_t* __restrict__ out) {
    using W = typename H::word;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    W key[16], st[8];
    key_from_row<H, H::kHash>(secrets + (uint64_t)H::kHash * i, key);
    hkdf_t1<H>(fin, key, st);
    digest_key<H>(st, key);
    Hm<H> h;
    hm_key<H>(key, h);
    const LabelPre none{};
    hm_row<H, false>(h, none, hashes + (uint64_t)H::kHash * i, H::kHash, st);
    store_digest<H>(st, out + (uint64_t)H::kHash * i);
}

// ---- tg_tls13_handshake_secrets --------------------------------------------------
// derived: HkdfLabel("derived", Hash(""), hash length); c / s: the bytes of
// "c hs traffic" / "s hs traffic" in front of the hello hash.
template <class H>
__global__ __launch_bounds__(256) void tls13_handshake_kernel(tg::HkdfMsg derived, LabelPre c, LabelPre s,
                                                              const uint8_t* __restrict__ psk,
                                                              const uint8_t* __restrict__ shared, uint32_t sharedlen,
                                                              const uint8_t* __restrict__ hello, uint64_t n,
                                                              uint8_t* __restrict__ hs_out,
                                                              uint8_t* __restrict__ c_out,
                                                              uint8_t* __restrict__ s_out) {
    using W = typename H::word;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LabelPre none{};
    W key[16], st[8], hs[8];
    Hm<H> h;
    key_from_row<H, H::kHash, true>(nullptr, key);                                   // early = Extract(0, psk or zeros)
    hm_key<H>(key, h);
    hm_row<H, false>(h, none, psk ? psk + (uint64_t)H::kHash * i : nullptr, H::kHash, st);
    digest_key<H>(st, key);                                     // Derive-Secret(early, "derived", Hash(""))
    hkdf_t1<H>(derived, key, st);
    digest_key<H>(st, key);                                     // hs = Extract(derived, shared)
    hm_key<H>(key, h);
    hm_row<H, false>(h, none, shared + (uint64_t)sharedlen * i, sharedlen, hs);
    digest_key<H>(hs, key);
    hm_key<H>(key, h);
    const uint8_t* hh = hello + (uint64_t)H::kHash * i;
    if (hs_out) store_digest<H>(hs, hs_out + (uint64_t)H::kHash * i);
    if (c_out) {
        hm_row<H, true>(h, c, hh, H::kHash, st);
        store_digest<H>(st, c_out + (uint64_t)H::kHash * i);
    }
    if (s_out) {
        hm_row<H, true>(h, s, hh, H::kHash, st);
        store_digest<H>(st, s_out + (uint64_t)H::kHash * i);
    }
}

// ---- tg_tls13_application_secrets ------------------------------------------------
// master_out may be the handshake secrets' own array: the lane's handshake
// secret is in registers before anything else happens, and all four stores
// come after the last load.  (No __restrict__ on the two that may alias.)
template <class H>
__global__ __launch_bounds__(256) void tls13_application_kernel(tg::HkdfMsg derived, LabelPre c, LabelPre s,
                                                                LabelPre e, const uint8_t* hs_in,
                                                                const uint8_t* __restrict__ fhash, uint64_t n,
                                                                uint8_t* master_out, uint8_t* __restrict__ c_out,
                                                                uint8_t* __restrict__ s_out,
                                                                uint8_t* __restrict__ e_out) {
    using W = typename H::word;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LabelPre none{};
    W key[16], st[8], ms[8], oc[8], os[8], oe[8];
    Hm<H> h;
    key_from_row<H, H::kHash>(hs_in + (uint64_t)H::kHash * i, key);            // Derive-Secret(hs, "derived", Hash(""))
    hkdf_t1<H>(derived, key, st);
    digest_key<H>(st, key);                                     // master = Extract(derived, zeros)
    hm_key<H>(key, h);
    hm_row<H, false>(h, none, nullptr, H::kHash, ms);
    digest_key<H>(ms, key);
    hm_key<H>(key, h);
    const uint8_t* fh = fhash + (uint64_t)H::kHash * i;
#pragma unroll
    for (int k = 0; k < 8; ++k) oc[k] = os[k] = oe[k] = 0;
    if (c_out) hm_row<H, true>(h, c, fh, H::kHash, oc);
    if (s_out) hm_row<H, true>(h, s, fh, H::kHash, os);
    if (e_out) hm_row<H, true>(h, e, fh, H::kHash, oe);
    if (master_out) store_digest<H>(ms, master_out + (uint64_t)H::kHash * i);
    if (c_out) store_digest<H>(oc, c_out + (uint64_t)H::kHash * i);
    if (s_out) store_digest<H>(os, s_out + (uint64_t)H::kHash * i);
    if (e_out) store_digest<H>(oe, e_out + (uint64_t)H::kHash * i);
}

// ---- host side -------------------------------------------------------------------
LabelPre label_pre(const uint8_t* label, size_t labellen, size_t ctxlen, size_t outlen) {
    uint8_t b[sizeof(LabelPre::w)] = {0};
    size_t at = 0;
    b[at++] = (uint8_t)(outlen >> 8);              // addTwo(length)
    b[at++] = (uint8_t)outlen;
    b[at++] = (uint8_t)(6 + labellen);             // addVarSeq("tls13 " + label, 1, 1)
    memcpy(b + at, "tls13 ", 6);
    at += 6;
    if (labellen) memcpy(b + at, label, labellen);
    at += labellen;
    b[at++] = (uint8_t)ctxlen;                     // addVarSeq(hashValue, 1, 1): its length byte
    LabelPre p{};
    p.len = (uint32_t)at;
    for (size_t k = 0; k < at; ++k) p.w[k / 4] |= (uint32_t)b[k] << (8 * (3 - k % 4));
    return p;
}

LabelPre label_pre(const char* label, int hashlen) {
    return label_pre((const uint8_t*)label, strlen(label), (size_t)hashlen, (size_t)hashlen);
}

// Hash(""), derive_secret's transcript for handshake_hashes None.
template <class H>
void empty_hash_of(uint8_t out[48]) {
    using W = typename H::word;
    W st[8], blk[16] = {0};
    blk[0] = (W)1 << (8 * sizeof(W) - 1);
    H::init(st);
    H::compress(st, blk);
    for (int k = 0; k < H::kHash; ++k)
        out[k] = (uint8_t)(st[k / sizeof(W)] >> (8 * (sizeof(W) - 1 - k % sizeof(W))));
}

void empty_hash(int hashlen, uint8_t out[48]) {
    if (hashlen == 32) empty_hash_of<Sha256>(out);
    else empty_hash_of<Sha384>(out);
}

// HkdfLabel(label, Hash(""), hashlen) or, with ctx false, HkdfLabel(label, "", hashlen).
int shared_message(int hashlen, const char* label, bool ctx, HkdfMsg* msg) {
    uint8_t eh[48];
    empty_hash(hashlen, eh);
    return host::hkdf_message(hashlen, (const uint8_t*)label, strlen(label), ctx ? eh : nullptr,
                              ctx ? (size_t)hashlen : 0, (size_t)hashlen, msg);
}

inline bool overlap(const uint8_t* a, const uint8_t* b, uint64_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + bytes && y < x + bytes;
}

#define TG_TLS13_LAUNCH(kernel, ...)                                                                      \
    do {                                                                                                  \
        if (hashlen == 32)                                                                                \
            hipLaunchKernelGGL(kernel<Sha256>, dim3(blocks_of(n)), dim3(256), 0, s, __VA_ARGS__);         \
        else                                                                                              \
            hipLaunchKernelGGL(kernel<Sha384>, dim3(blocks_of(n)), dim3(256), 0, s, __VA_ARGS__);         \
    } while (0)

}  // namespace
}  // namespace tg

using tg::fail;

extern "C" {

int tg_hkdf_extract(int hashlen, const uint8_t* salts, const uint8_t* ikm, size_t ikmlen, uint64_t n, uint8_t* out,
                    void* stream) {
    using namespace tg;
    if (hashlen != 32 && hashlen != 48) return fail(TG_EINVAL, "hash length must be 32 or 48");
    if (!ikm && ikmlen != 0 && ikmlen != (size_t)hashlen)
        return fail(TG_EINVAL, "a null ikm stands for %d zero bytes: ikm length must be 0 or %d, got %zu", hashlen,
                    hashlen, ikmlen);
    if (ikm && (ikmlen == 0 || ikmlen > 1024))
        return fail(TG_EINVAL, "ikm length must be 1..1024, got %zu", ikmlen);
    if (n > kMaxSessions) return fail(TG_EINVAL, "n must be at most 2^31");
    if (n == 0) return TG_OK;
    if (!out) return fail(TG_EINVAL, "null device buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TG_TLS13_LAUNCH(tls13_extract_kernel, salts, ikm, (uint32_t)(ikm ? ikmlen : (size_t)hashlen), n, out);
    return launched() ? TG_OK : fail(TG_EHIP, "extract launch failed");
}

int tg_hkdf_expand_label_rows(int hashlen, const uint8_t* secrets, uint64_t n, const uint8_t* label, size_t labellen,
                              const uint8_t* contexts, size_t ctxlen, size_t outlen, uint8_t* out, void* stream) {
    using namespace tg;
    if (hashlen != 32 && hashlen != 48) return fail(TG_EINVAL, "hash length must be 32 or 48");
    if (labellen > 32) return fail(TG_EINVAL, "label length must be at most 32, got %zu", labellen);
    if (ctxlen > 64) return fail(TG_EINVAL, "context length must be at most 64, got %zu", ctxlen);
    if (outlen == 0 || outlen > (size_t)hashlen)
        return fail(TG_EINVAL, "output length must be 1..%d, got %zu", hashlen, outlen);
    if (labellen && !label) return fail(TG_EINVAL, "null label");
    if (!contexts && ctxlen != 0 && ctxlen != (size_t)hashlen)
        return fail(TG_EINVAL, "null contexts stand for the empty transcript's hash: context length must be 0 or %d, "
                               "got %zu", hashlen, ctxlen);
    if (n > kMaxSessions) return fail(TG_EINVAL, "n must be at most 2^31");
    if (n == 0) return TG_OK;
    if (!secrets || !out) return fail(TG_EINVAL, "null device buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!contexts && ctxlen) {   // Hash(""): one context for all rows, hkdf_kernel's case
        uint8_t eh[48];
        empty_hash(hashlen, eh);
        HkdfMsg msg;
        if (host::hkdf_message(hashlen, label, labellen, eh, ctxlen, outlen, &msg))
            return fail(TG_EINVAL, "label + context too long");
        const int rc = tg_launch_hkdf(hashlen, msg, secrets, n, out, s);
        return rc ? fail(rc, "hkdf launch failed") : TG_OK;
    }
    const LabelPre pre = label_pre(label, labellen, ctxlen, outlen);
    TG_TLS13_LAUNCH(tls13_expand_rows_kernel, pre, secrets, contexts, (uint32_t)ctxlen, n, (uint32_t)outlen, out);
    return launched() ? TG_OK : fail(TG_EHIP, "expand-label launch failed");
}

int tg_tls13_finished(int hashlen, const uint8_t* secrets, const uint8_t* hashes, uint64_t n, uint8_t* out,
                      void* stream) {
    using namespace tg;
    if (hashlen != 32 && hashlen != 48) return fail(TG_EINVAL, "hash length must be 32 or 48");
    if (n > kMaxSessions) return fail(TG_EINVAL, "n must be at most 2^31");
    if (n == 0) return TG_OK;
    if (!secrets || !hashes || !out) return fail(TG_EINVAL, "null device buffer");
    HkdfMsg fin;
    if (shared_message(hashlen, "finished", false, &fin)) return fail(TG_EINVAL, "label too long");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TG_TLS13_LAUNCH(tls13_finished_kernel, fin, secrets, hashes, n, out);
    return launched() ? TG_OK : fail(TG_EHIP, "finished launch failed");
}

int tg_tls13_handshake_secrets(int hashlen, const uint8_t* psk, const uint8_t* shared, size_t sharedlen,
                               const uint8_t* hello_hash, uint64_t n, uint8_t* handshake_secret,
                               uint8_t* client_traffic, uint8_t* server_traffic, void* stream) {
    using namespace tg;
    if (hashlen != 32 && hashlen != 48) return fail(TG_EINVAL, "hash length must be 32 or 48");
    if (sharedlen == 0 || sharedlen > 1024)
        return fail(TG_EINVAL, "shared secret length must be 1..1024, got %zu", sharedlen);
    if (!handshake_secret && !client_traffic && !server_traffic)
        return fail(TG_EINVAL, "no output: handshake_secret, client_traffic and server_traffic are all null");
    if (n > kMaxSessions) return fail(TG_EINVAL, "n must be at most 2^31");
    if (n == 0) return TG_OK;
    if (!shared || !hello_hash) return fail(TG_EINVAL, "null device buffer");
    HkdfMsg derived;
    if (shared_message(hashlen, "derived", true, &derived)) return fail(TG_EINVAL, "label too long");
    const LabelPre c = label_pre("c hs traffic", hashlen), sv = label_pre("s hs traffic", hashlen);
    hipStream_t s = static_cast<hipStream_t>(stream);
    TG_TLS13_LAUNCH(tls13_handshake_kernel, derived, c, sv, psk, shared, (uint32_t)sharedlen, hello_hash, n,
                    handshake_secret, client_traffic, server_traffic);
    return launched() ? TG_OK : fail(TG_EHIP, "handshake stage launch failed");
}

int tg_tls13_application_secrets(int hashlen, const uint8_t* handshake_secret, const uint8_t* finished_hash,
                                 uint64_t n, uint8_t* master_secret, uint8_t* client_traffic, uint8_t* server_traffic,
                                 uint8_t* exporter_master, void* stream) {
    using namespace tg;
    if (hashlen != 32 && hashlen != 48) return fail(TG_EINVAL, "hash length must be 32 or 48");
    if (!master_secret && !client_traffic && !server_traffic && !exporter_master)
        return fail(TG_EINVAL, "no output: master_secret, client_traffic, server_traffic and exporter_master are "
                               "all null");
    if (n > kMaxSessions) return fail(TG_EINVAL, "n must be at most 2^31");
    if (n == 0) return TG_OK;
    if (!handshake_secret || !finished_hash) return fail(TG_EINVAL, "null device buffer");
    const uint64_t bytes = n * (uint64_t)hashlen;
    const uint8_t* outs[4] = {master_secret, client_traffic, server_traffic, exporter_master};
    for (int a = 0; a < 4; ++a) {
        if (overlap(outs[a], finished_hash, bytes) ||
            (overlap(outs[a], handshake_secret, bytes) && !(a == 0 && master_secret == handshake_secret)))
            return fail(TG_EINVAL, "an output overlaps an input (only master_secret == handshake_secret may)");
        for (int b = a + 1; b < 4; ++b)
            if (overlap(outs[a], outs[b], bytes)) return fail(TG_EINVAL, "two outputs overlap");
    }
    HkdfMsg derived;
    if (shared_message(hashlen, "derived", true, &derived)) return fail(TG_EINVAL, "label too long");
    const LabelPre c = label_pre("c ap traffic", hashlen), sv = label_pre("s ap traffic", hashlen),
                   e = label_pre("exp master", hashlen);
    hipStream_t s = static_cast<hipStream_t>(stream);
    TG_TLS13_LAUNCH(tls13_application_kernel, derived, c, sv, e, handshake_secret, finished_hash, n, master_secret,
                    client_traffic, server_traffic, exporter_master);
    return launched() ? TG_OK : fail(TG_EHIP, "application stage launch failed");
}

}  // extern "C"
