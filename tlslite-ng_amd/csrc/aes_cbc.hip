// aes_cbc.hip -- batched TLS 1.1 / 1.2 AES-CBC + HMAC records for gfx950:
// the key handles (tg_cbc_key_create / _create_table / _info / _replace /
// _destroy) and one connection direction per call (tg_cbc_seal_records,
// tg_cbc_open_records).  The record arithmetic is cbc_dev.h's, shared with the
// session-per-record kernels of aes_cbc_table.hip.
//
// Restates the block-cipher paths of tlslite/recordlayer.py for TLS >= 1.1,
// one record per lane:
//   _macThenEncrypt :476-498    header || IV || CBC(data || MAC || padding)
//   _encryptThenMAC :500-520    header || IV || CBC(data || padding) || MAC
//   _decryptThenMAC :680-719    with ct_check_cbc_mac_and_pad
//                               (constanttime.py:102-204)
//   _macThenDecrypt :721-778    RFC 7366
//   addPadding :453-461, calculateMAC :463-474, and the length limits of
//   RecordSocket.recv :219-220 and recvRecord :980-981.
// The reference chains the records of a connection through its cipher object
// and prepends a random block; the first ciphertext block is then an explicit
// IV and the rest is CBC under that IV, so the records of a batch are
// independent given one IV per record (tg_cbc_records.iv).
//
// Layout.  A lane owns a record and runs its two serial chains one after the
// other -- the hash (64 / 80 rounds per 64- / 128-byte block) and CBC (ten or
// fourteen table rounds per 16-byte block):
//   MtE seal   HMAC over the fragment, MAC and padding written behind it in
//              the wire buffer, then CBC over fragment || MAC || padding
//   EtM seal   CBC, then HMAC over the IV and ciphertext just written
//   MtE open   P_j = D(C_j) ^ C_(j-1) into the caller's data buffer, then the
//              constant-work verdict over it (cbc_record.h)
//   EtM open   HMAC over the wire bytes, then decryption and the padding check
// Both chains are serial within a record and parallel across records, so a
// batch fills the machine only with tens of thousands of records (one lane
// each); batches too small for that are not this file's concern -- there is
// no wave-per-record kernel here.  The second pass re-reads the record from
// L2 rather than interleaving the chains: the hash state (SHA-384: sixteen
// 64-bit message words and sixteen state words) and the cipher state are
// then never live together, and no instantiation spills.
//
// LDS: a seal kernel stages the 64 KiB Te0 / Te2 copy block of aes_round.h,
// an open kernel the same layout filled with Td0 / Td2 (the equivalent
// inverse cipher: the column formula of aes_round.h col() holds with the
// state words taken in InvShiftRows order) plus 16 KiB of inverse S-box
// copies for the last round (row x = 16 copies of Si[x]; lanes l and l + 16
// share a bank, a two-way conflict on 16 of a block's 160 lookups).  512
// threads per workgroup, two workgroups per CU (128 / 160 KiB of LDS).  The
// round keys (seal: the schedule, open: the inverse schedule with
// InvMixColumns applied to rounds 1 .. Nr - 1) are wave-uniform in SGPRs.
#include "api.h"
#include "cbc_dev.h"
#include "runtime.h"

#include <stdio.h>
#include <string.h>

#include <new>

namespace tg {
namespace {

// ---- seal ------------------------------------------------------------------
template <int NR, class H, bool ETM>
__global__ __launch_bounds__(kCbcThreads) void cbc_seal_kernel(const CbcKeyDev* __restrict__ key,
                                                               tg_cbc_records r) {
    stage_te(reinterpret_cast<uint32_t*>(g_lds_cbc));   // Te0/Te2 copies at LDS 0
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.n) return;
    RkRegs<NR> rk;
#pragma unroll
    for (int k = 0; k < 4 * (NR + 1); ++k) rk.w[k] = key->ek[k];
    const uint32_t lane4 = (threadIdx.x & 31u) << 2;
    constexpr uint32_t D = H::kHash;

    const uint32_t len = gld(r.data_len, i);
    const uint8_t* src = r.data + gld(r.data_off, i);
    uint8_t* w = r.wire + gld(r.wire_off, i);
    const uint32_t type = gld(r.ctype, i);
    const uint64_t seq = r.seq0 + i;
    // addPadding (:453-461): up to the next multiple of 16 past one length byte
    const uint32_t enc = ETM ? ((len + 16u) & ~15u) : ((len + D + 16u) & ~15u);
    const uint32_t body = 16u + enc + (ETM ? D : 0u);
    uint8_t* ct = w + 21;
    const bool aligned = (((uintptr_t)src | (uintptr_t)ct) & 15) == 0;
    const uint32_t nfull = len >> 4, tail = len & 15;

    const gptr hw = (gptr)w;
    hw[0] = (uint8_t)type;
    hw[1] = (uint8_t)(r.version >> 8);
    hw[2] = (uint8_t)r.version;
    hw[3] = (uint8_t)(body >> 8);
    hw[4] = (uint8_t)body;
    uint4 prev = gload16u(r.iv + 16 * i);
    store16(w + 5, prev, aligned);

    uint32_t dig[12];
    if (!ETM) {
        cbc::hmac_record<H, GMem>(key->mid, seq, type, r.version, src, len, len, cbc::hmac_blocks<H>(len), dig);
        // the plaintext behind the last whole fragment block, in place: the
        // fragment's last bytes, the MAC, the padding
        if (tail) store_partial(ct + 16 * nfull, load_partial(src + 16 * nfull, tail), tail);
        store_mac<H>(ct + len, dig);
        const uint32_t padv = enc - len - D - 1u;
        const gptr pp = (gptr)ct;
        for (uint32_t k = len + D; k < enc; ++k) pp[k] = (uint8_t)padv;
        for (uint32_t j = 0; j < enc >> 4; ++j) {
            const uint4 p = j < nfull ? load16(src + 16 * j, aligned) : load16(ct + 16 * j, aligned);
            prev = aes_block<NR>(lane4, rk, xor4(p, prev));
            store16(ct + 16 * j, prev, aligned);
        }
    } else {
        for (uint32_t j = 0; j < nfull; ++j) {
            prev = aes_block<NR>(lane4, rk, xor4(load16(src + 16 * j, aligned), prev));
            store16(ct + 16 * j, prev, aligned);
        }
        const uint32_t pad4 = (15u - tail) * 0x01010101u;
        const uint4 pads = make_uint4(pad4, pad4, pad4, pad4);
        const uint4 last = xor4(xor4(pads, mask_tail(pads, tail)), load_partial(src + 16 * nfull, tail));
        prev = aes_block<NR>(lane4, rk, xor4(last, prev));
        store16(ct + 16 * nfull, prev, aligned);
        // MAC over IV || ciphertext (:511-518)
        cbc::hmac_record<H, GMem>(key->mid, seq, type, r.version, w + 5, 16u + enc, 16u + enc,
                                  cbc::hmac_blocks<H>(16u + enc), dig);
        store_mac<H>(ct + enc, dig);
    }
    gst(r.wire_len, i, 5u + body);
}

// ---- open ------------------------------------------------------------------
// CBC decryption of n bytes (a multiple of 16) at c, whose previous block
// (the IV) sits right in front of it.
template <int NR>
__device__ __forceinline__ void cbc_decrypt(uint32_t lane4, uint32_t si4, const RkRegs<NR>& dk,
                                            const uint8_t* c, uint8_t* out, uint32_t n, bool aligned) {
    uint4 prev = load16(c - 16, aligned);
    for (uint32_t k = 0; k < n; k += 16) {
        const uint4 cur = load16(c + k, aligned);
        store16(out + k, xor4(aes_dec_block<NR>(lane4, si4, dk, cur), prev), aligned);
        prev = cur;
    }
}

template <int NR, class H, bool ETM>
__global__ __launch_bounds__(kCbcThreads) void cbc_open_kernel(const CbcKeyDev* __restrict__ key,
                                                               tg_cbc_records r) {
    stage_td(g_lds_cbc);
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.n) return;
    RkRegs<NR> dk;
#pragma unroll
    for (int k = 0; k < 4 * (NR + 1); ++k) dk.w[k] = key->dk[k];
    const uint32_t lane4 = (threadIdx.x & 31u) << 2, si4 = (threadIdx.x & 15u) << 2;
    constexpr uint32_t D = H::kHash;

    const uint32_t wl = gld(r.wire_len, i);
    const uint8_t* w = r.wire + gld(r.wire_off, i);
    uint8_t* out = r.data + gld(r.data_off, i);
    const uint64_t seq = r.seq0 + i;
    const uint32_t limit = r.recv_limit ? r.recv_limit : 16384u;
    const bool aligned = (((uintptr_t)out | (uintptr_t)(w + 5)) & 15) == 0;

    uint32_t st = TG_REC_OK, plen = 0, type = 0;
    uint32_t wrote = 0;                                   // bytes of ``out`` holding decrypted data
    if (wl < 5) {
        st = TG_REC_BAD_MAC;                              // not even a header: nothing to authenticate
    } else {
        const gptr_c hw = (gptr_c)w;
        type = hw[0];
        const uint32_t hlen = ((uint32_t)hw[3] << 8) | hw[4];
        const uint32_t body = wl - 5;
        if (!ETM) {
            st = cbc::mte_public_status(D, hlen, body, limit);
            if (st == TG_REC_OK) {
                const uint32_t n = body - 16u;
                cbc_decrypt<NR>(lane4, si4, dk, w + 21, out, n, aligned);
                wrote = n;
                st = cbc::final_status(cbc::mte_verdict<H, GMem>(key->mid, seq, type, r.version, out, n, &plen),
                                       plen, limit);
            }
        } else if (hlen > limit + 2048u || body > limit + 2048u) {
            st = TG_REC_OVERFLOW;                         // RecordSocket.recv :219-220
        } else {
            if (body < D) {
                st = TG_REC_BAD_MAC;                      // "Truncated data" :730-731
            } else {
                const uint32_t bl = body - D;
                uint32_t dig[12];
                cbc::hmac_record<H, GMem>(key->mid, seq, type, r.version, w + 5, bl, bl, cbc::hmac_blocks<H>(bl), dig);
                const uint32_t n = bl >= 16u ? bl - 16u : 0u;
                if (cbc::mac_differs<H, GMem>(w + 5 + bl, dig)) {
                    st = TG_REC_BAD_MAC;                  // :741-742
                } else if (bl & 15u) {
                    st = TG_REC_DECRYPT_FAILED;           // :746-748
                } else if (n == 0) {
                    st = TG_REC_BAD_MAC;                  // "No data left after IV removal" :756-757
                } else {
                    cbc_decrypt<NR>(lane4, si4, dk, w + 21, out, n, aligned);
                    wrote = n;
                    if (cbc::etm_padding<GMem>(out, n, &plen)) st = TG_REC_BAD_MAC;   // :759-773
                }
            }
        }
        if (ETM && st == TG_REC_OK) st = cbc::final_status(0, plen, limit);   // recvRecord :980-981
    }
    if (st != TG_REC_OK) {
        zero_bytes(out, wrote, aligned);                  // no unauthenticated plaintext stays behind
        plen = 0;
    }
    gst(r.status, i, (uint8_t)st);
    gst(r.data_len, i, plen);
    gst(r.ctype, i, (uint8_t)type);
}

template <int NR, class H, bool ETM>
int launch2(const CbcKeyDev* key, const tg_cbc_records& r, bool open, hipStream_t s) {
    const uint64_t blocks = (r.n + kCbcThreads - 1) / kCbcThreads;
    if (blocks > 0x7fffffffull) return fail(TG_EINVAL, "too many records");
    if (open) {
        if (lds_attr((const void*)cbc_open_kernel<NR, H, ETM>, (int)kOpenLds)) return fail(TG_EHIP, "LDS attribute");
        hipLaunchKernelGGL((cbc_open_kernel<NR, H, ETM>), dim3((unsigned)blocks), dim3(kCbcThreads), kOpenLds, s,
                           key, r);
    } else {
        if (lds_attr((const void*)cbc_seal_kernel<NR, H, ETM>, (int)kSealLds)) return fail(TG_EHIP, "LDS attribute");
        hipLaunchKernelGGL((cbc_seal_kernel<NR, H, ETM>), dim3((unsigned)blocks), dim3(kCbcThreads), kSealLds, s,
                           key, r);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TG_OK : fail(TG_EHIP, "cbc kernel launch: %s", hipGetErrorString(e));
}

template <int NR, class H>
int launch1(const CbcKeyDev* key, const tg_cbc_records& r, bool open, hipStream_t s) {
    return r.etm ? launch2<NR, H, true>(key, r, open, s) : launch2<NR, H, false>(key, r, open, s);
}

template <int NR>
int launch0(int mac, const CbcKeyDev* key, const tg_cbc_records& r, bool open, hipStream_t s) {
    switch (mac) {
        case TG_MAC_SHA1: return launch1<NR, Sha1>(key, r, open, s);
        case TG_MAC_SHA256: return launch1<NR, Sha256>(key, r, open, s);
        default: return launch1<NR, Sha384>(key, r, open, s);
    }
}

void scrub(void* p, size_t n) {
    volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) v[k] = 0;
}

int cbc_records(tg_cbc_key* k, const tg_cbc_records* r, void* stream, bool open) {
    // argument errors first, before any HIP call; those of the struct alone
    // are reported whatever the key is
    if (!r) return fail(TG_EINVAL, "null tg_cbc_records");
    if (r->version != TG_TLS11 && r->version != TG_TLS12)
        return fail(TG_EINVAL, "version 0x%04x is neither TG_TLS11 nor TG_TLS12", r->version);
    if (r->etm > 1) return fail(TG_EINVAL, "etm must be 0 or 1, got %u", r->etm);
    if (!open && !r->iv) return fail(TG_EINVAL, "seal needs iv (16 bytes per record)");
    if (!k) return fail(TG_EINVAL, "null key");
    if (r->n == 0) return TG_OK;
    if (!r->data || !r->data_off || !r->data_len || !r->ctype || !r->wire || !r->wire_off || !r->wire_len)
        return fail(TG_EINVAL, "null device array");
    if (open && !r->status) return fail(TG_EINVAL, "open needs status");
    if (int rc = cbc_select_device(k)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return k->rounds == 10 ? launch0<10>(k->mac, k->dev_key, *r, open, s)
                           : launch0<14>(k->mac, k->dev_key, *r, open, s);
}

// ---- key handles: one row, or a table of them -------------------------------
constexpr size_t kStageRows = 1024;   // tg_cbc_key_replace's pinned staging (624 KiB)

// The device row of one (cipher key, MAC key) pair, built on the host.
void build_row(const uint8_t* enc_key, size_t keylen, const uint8_t* mac_key, size_t mackeylen, int mac,
               CbcKeyDev* img) {
    const int nr = host::aes_round_words(enc_key, keylen, img->ek, nullptr);
    for (int r = 0; r <= nr; ++r)
        for (int c = 0; c < 4; ++c) {
            const uint32_t w = img->ek[4 * (nr - r) + c];
            img->dk[4 * r + c] = (r == 0 || r == nr) ? w : inv_mix_column(w);
        }
    if (mac == TG_MAC_SHA1) cbc::hmac_midstates<Sha1>(mac_key, (uint32_t)mackeylen, &img->mid);
    else if (mac == TG_MAC_SHA256) cbc::hmac_midstates<Sha256>(mac_key, (uint32_t)mackeylen, &img->mid);
    else cbc::hmac_midstates<Sha384>(mac_key, (uint32_t)mackeylen, &img->mid);
    img->rounds = (uint32_t)nr;
    img->mac = (uint32_t)mac;
}

int key_create(const uint8_t* enc_keys, size_t keylen, const uint8_t* mac_keys, size_t mackeylen, int mac,
               size_t nkeys, tg_cbc_key** out) {
    if (!out || !enc_keys || !mac_keys) return fail(TG_EINVAL, "null argument");
    char buf[80];
    if (const char* msg = table_error(keylen, mackeylen, mac, nkeys, buf)) return fail(TG_EINVAL, "%s", msg);

    CbcKeyDev* img = new (std::nothrow) CbcKeyDev[nkeys]();
    tg_cbc_key* k = new (std::nothrow) tg_cbc_key();
    if (!img || !k) {
        delete[] img;
        delete k;
        return fail(TG_ENOMEM, "out of host memory");
    }
    for (size_t j = 0; j < nkeys; ++j)
        build_row(enc_keys + j * keylen, keylen, mac_keys + j * mackeylen, mackeylen, mac, img + j);
    k->rounds = keylen == 16 ? 10 : 14;
    k->mac = mac;
    k->nkeys = nkeys;
    k->dev_key = nullptr;
    k->stage = nullptr;
    k->stage_done = nullptr;
    hipError_t e = hipGetDevice(&k->device);
    if (e == hipSuccess) e = hipMalloc((void**)&k->dev_key, nkeys * sizeof(CbcKeyDev));
    if (e == hipSuccess) e = hipMemcpy(k->dev_key, img, nkeys * sizeof(CbcKeyDev), hipMemcpyHostToDevice);
    scrub(img, nkeys * sizeof(CbcKeyDev));
    delete[] img;
    if (e != hipSuccess) {
        if (k->dev_key) (void)hipFree(k->dev_key);
        delete k;
        return fail(TG_EHIP, "cbc key upload: %s", hipGetErrorString(e));
    }
    *out = k;
    return TG_OK;
}

// tg_cbc_key_replace.  The rows are built in pinned staging, kStageRows at a
// time; each run of consecutive slots is one copy on the stream; the host
// waits on an event behind a chunk's copies (not on the device) and scrubs
// the staging before it is filled again or the call returns.
int key_replace(tg_cbc_key* k, const uint32_t* slot, const uint8_t* enc_keys, const uint8_t* mac_keys,
                size_t mackeylen, uint64_t n, hipStream_t s) {
    const size_t keylen = k->rounds == 10 ? 16 : 32;
    if (int rc = cbc_select_device(k)) return rc;
    if (!k->stage) {
        HIP_TRY(hipHostMalloc((void**)&k->stage, kStageRows * sizeof(CbcKeyDev), hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&k->stage_done, hipEventDisableTiming));
    }
    for (uint64_t base = 0; base < n; base += kStageRows) {
        const size_t m = (size_t)(n - base < kStageRows ? n - base : kStageRows);
        hipError_t e = hipSuccess;
        for (size_t j = 0; j < m && e == hipSuccess;) {
            const uint64_t first = slot ? slot[base + j] : base + j;
            if (first >= k->nkeys) {   // skipped: nothing of the table is touched
                ++j;
                continue;
            }
            size_t run = 0;
            while (j + run < m && (slot ? slot[base + j + run] : base + j + run) == first + run &&
                   first + run < k->nkeys) {
                const uint64_t row = base + j + run;
                build_row(enc_keys + row * keylen, keylen, mac_keys + row * mackeylen, mackeylen, k->mac,
                          k->stage + j + run);
                ++run;
            }
            e = hipMemcpyAsync(k->dev_key + first, k->stage + j, run * sizeof(CbcKeyDev), hipMemcpyHostToDevice,
                               s);
            j += run;
        }
        if (e == hipSuccess) e = hipEventRecord(k->stage_done, s);
        if (e == hipSuccess) e = hipEventSynchronize(k->stage_done);
        else (void)hipStreamSynchronize(s);   // copies already queued must be done with the staging
        scrub(k->stage, m * sizeof(CbcKeyDev));
        if (e != hipSuccess) return fail(TG_EHIP, "cbc key replace: %s", hipGetErrorString(e));
    }
    return TG_OK;
}

}  // namespace
}  // namespace tg

using tg::fail;

extern "C" {

int tg_cbc_key_create(const uint8_t* enc_key, size_t keylen, const uint8_t* mac_key, size_t mackeylen, int mac,
                      tg_cbc_key** out) {
    return tg::key_create(enc_key, keylen, mac_key, mackeylen, mac, 1, out);
}

int tg_cbc_key_create_table(const uint8_t* enc_keys, size_t keylen, const uint8_t* mac_keys, size_t mackeylen,
                            int mac, size_t nkeys, tg_cbc_key** out) {
    return tg::key_create(enc_keys, keylen, mac_keys, mackeylen, mac, nkeys, out);
}

int tg_cbc_key_info(const tg_cbc_key* k, size_t* keylen, int* mac, size_t* nkeys) {
    if (!k) return fail(TG_EINVAL, "null key");
    if (keylen) *keylen = k->rounds == 10 ? 16 : 32;
    if (mac) *mac = k->mac;
    if (nkeys) *nkeys = k->nkeys;
    return TG_OK;
}

int tg_cbc_key_replace(tg_cbc_key* k, const uint32_t* slot, const uint8_t* enc_keys, const uint8_t* mac_keys,
                       size_t mackeylen, uint64_t n, void* stream) {
    if (!k) return fail(TG_EINVAL, "null key");
    if (n > k->nkeys)
        return fail(TG_EINVAL, "%llu rows for a table of %zu keys", (unsigned long long)n, k->nkeys);
    if (n == 0) return TG_OK;
    if (!enc_keys || !mac_keys) return fail(TG_EINVAL, "null argument");
    char buf[80];
    if (const char* msg = tg::key_error(k->rounds == 10 ? 16 : 32, mackeylen, k->mac, buf))
        return fail(TG_EINVAL, "%s", msg);
    return tg::key_replace(k, slot, enc_keys, mac_keys, mackeylen, n, static_cast<hipStream_t>(stream));
}

int tg_cbc_key_destroy(tg_cbc_key* k) {
    if (!k) return TG_OK;
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != k->device) (void)hipSetDevice(k->device);
    // batches may still be reading the rows on callers' streams
    (void)hipDeviceSynchronize();
    if (k->dev_key) {
        (void)hipMemset(k->dev_key, 0, k->nkeys * sizeof(tg::CbcKeyDev));
        (void)hipFree(k->dev_key);
    }
    if (k->stage) (void)hipHostFree(k->stage);   // scrubbed at the end of every replace
    if (k->stage_done) (void)hipEventDestroy(k->stage_done);
    delete k;
    return TG_OK;
}

int tg_cbc_seal_records(tg_cbc_key* k, const tg_cbc_records* r, void* stream) {
    return tg::cbc_records(k, r, stream, false);
}

int tg_cbc_open_records(tg_cbc_key* k, const tg_cbc_records* r, void* stream) {
    return tg::cbc_records(k, r, stream, true);
}

}  // extern "C"
