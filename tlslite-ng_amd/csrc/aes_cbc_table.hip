// aes_cbc_table.hip -- AES-CBC + HMAC records of many sessions in one batch:
// tg_cbc_seal_session_records / tg_cbc_open_session_records.
//
// The pending CBC records of many RecordLayers (one direction each) through
// one call: record i is sealed / opened under row session[i] of the handle's
// key table with a per-session sequence number -- the caller's (seq) or the
// session's counter plus the record's stable rank in the batch (seq_next,
// sessions.hip).  Per record everything is aes_cbc.hip's.  The hash and verdict
// arithmetic is one piece of code for both paths (cbc_record.h: hmac_record,
// mte_verdict, etm_padding, mac_differs, called unchanged, so its constant-work
// property covers this path), and so are the cipher rounds and memory helpers
// (aes_round.h, cbc_dev.h).  seal_record / open_record below repeat the text
// of the single-key kernels around them rather than share it: those kernels
// keep their own text so that they assemble to the same instructions as
// before this file existed (a shared body, inlined one level deeper, did not
// -- DESIGN.md 3.16).  A change to one must be made to the other;
// tests/test_gpu_cbc_sessions.py compares the two paths byte for byte.
//
// What differs is where the keys come from.  With a session per lane neither
// the round keys nor the HMAC midstates are wave-uniform: they are vector
// loads from the lane's row.  The LDS is taken by the tables (64 / 80 KiB at
// two workgroups per CU), so a lane's schedule lives in VGPRs: RkRow names
// the row, and cipher_keys() loads its 11 / 15 round keys (44 / 60 registers)
// at the start of the record's cipher pass -- after the hash pass of a
// MAC-then-encrypt seal, before the hash pass of a MAC-then-encrypt open --
// so the schedule and the hash's message block are never live together.  The
// midstates are read where hmac_record starts from them.  Register counts and
// the measured cost against the single-key kernels: DESIGN.md 3.16.
//
// A record whose session is out of range is skipped before anything else of
// it is read: the test comes first in both kernels.
#include "api.h"
#include "cbc_dev.h"
#include "runtime.h"

namespace tg {
namespace {

// A lane's schedule in its session's row (ek or dk: 16-byte aligned).
template <int NR>
struct RkRow {
    const uint4* row;
};

// The schedule in this lane's registers.
template <int NR>
struct RkVec {
    uint4 k[NR + 1];
    __device__ __forceinline__ uint4 get(int r) const { return k[r]; }
};

template <int NR>
__device__ __forceinline__ RkVec<NR> cipher_keys(const RkRow<NR>& src) {
    RkVec<NR> v;
#pragma unroll
    for (int r = 0; r <= NR; ++r) v.k[r] = src.row[r];
    return v;
}

// ---- seal ------------------------------------------------------------------
// Record i of r under row ``key`` and sequence number seq: the text of
// cbc_seal_kernel (aes_cbc.hip) with the lane's own keys.
template <int NR, class H, bool ETM>
__device__ __forceinline__ void seal_record(const CbcKeyDev* key, uint64_t seq, uint64_t i,
                                            const tg_cbc_session_records& r) {
    const RkRow<NR> rk{reinterpret_cast<const uint4*>(key->ek)};
    const cbc::Mid& mid = key->mid;
    const uint32_t lane4 = (threadIdx.x & 31u) << 2;
    constexpr uint32_t D = H::kHash;

    const uint32_t len = gld(r.data_len, i);
    const uint8_t* src = r.data + gld(r.data_off, i);
    uint8_t* w = r.wire + gld(r.wire_off, i);
    const uint32_t type = gld(r.ctype, i);
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
        cbc::hmac_record<H, GMem>(mid, seq, type, r.version, src, len, len, cbc::hmac_blocks<H>(len), dig);
        // the plaintext behind the last whole fragment block, in place: the
        // fragment's last bytes, the MAC, the padding
        if (tail) store_partial(ct + 16 * nfull, load_partial(src + 16 * nfull, tail), tail);
        store_mac<H>(ct + len, dig);
        const uint32_t padv = enc - len - D - 1u;
        const gptr pp = (gptr)ct;
        for (uint32_t k = len + D; k < enc; ++k) pp[k] = (uint8_t)padv;
        const RkVec<NR> ck = cipher_keys(rk);
        for (uint32_t j = 0; j < enc >> 4; ++j) {
            const uint4 p = j < nfull ? load16(src + 16 * j, aligned) : load16(ct + 16 * j, aligned);
            prev = aes_block<NR>(lane4, ck, xor4(p, prev));
            store16(ct + 16 * j, prev, aligned);
        }
    } else {
        {
            const RkVec<NR> ck = cipher_keys(rk);
            for (uint32_t j = 0; j < nfull; ++j) {
                prev = aes_block<NR>(lane4, ck, xor4(load16(src + 16 * j, aligned), prev));
                store16(ct + 16 * j, prev, aligned);
            }
            const uint32_t pad4 = (15u - tail) * 0x01010101u;
            const uint4 pads = make_uint4(pad4, pad4, pad4, pad4);
            const uint4 last = xor4(xor4(pads, mask_tail(pads, tail)), load_partial(src + 16 * nfull, tail));
            prev = aes_block<NR>(lane4, ck, xor4(last, prev));
            store16(ct + 16 * nfull, prev, aligned);
        }
        // MAC over IV || ciphertext (:511-518)
        cbc::hmac_record<H, GMem>(mid, seq, type, r.version, w + 5, 16u + enc, 16u + enc,
                                  cbc::hmac_blocks<H>(16u + enc), dig);
        store_mac<H>(ct + enc, dig);
    }
    gst(r.wire_len, i, 5u + body);
}

// ---- open ------------------------------------------------------------------
// CBC decryption of n bytes (a multiple of 16) at c, whose previous block
// (the IV) sits right in front of it.
template <int NR>
__device__ __forceinline__ void cbc_decrypt(uint32_t lane4, uint32_t si4, const RkRow<NR>& dk,
                                            const uint8_t* c, uint8_t* out, uint32_t n, bool aligned) {
    const RkVec<NR> ck = cipher_keys(dk);
    uint4 prev = load16(c - 16, aligned);
    for (uint32_t k = 0; k < n; k += 16) {
        const uint4 cur = load16(c + k, aligned);
        store16(out + k, xor4(aes_dec_block<NR>(lane4, si4, ck, cur), prev), aligned);
        prev = cur;
    }
}

// Record i of r under row ``key`` and sequence number seq: the text of
// cbc_open_kernel (aes_cbc.hip) with the lane's own keys.
template <int NR, class H, bool ETM>
__device__ __forceinline__ void open_record(const CbcKeyDev* key, uint64_t seq, uint64_t i,
                                            const tg_cbc_session_records& r) {
    const RkRow<NR> dk{reinterpret_cast<const uint4*>(key->dk)};
    const cbc::Mid& mid = key->mid;
    const uint32_t lane4 = (threadIdx.x & 31u) << 2, si4 = (threadIdx.x & 15u) << 2;
    constexpr uint32_t D = H::kHash;

    const uint32_t wl = gld(r.wire_len, i);
    const uint8_t* w = r.wire + gld(r.wire_off, i);
    uint8_t* out = r.data + gld(r.data_off, i);
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
                st = cbc::final_status(cbc::mte_verdict<H, GMem>(mid, seq, type, r.version, out, n, &plen),
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
                cbc::hmac_record<H, GMem>(mid, seq, type, r.version, w + 5, bl, bl, cbc::hmac_blocks<H>(bl), dig);
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
__global__ __launch_bounds__(kCbcThreads) void cbctab_seal(const CbcKeyDev* __restrict__ tab,
                                                           tg_cbc_session_records r,
                                                           const uint64_t* __restrict__ seq) {
    stage_te(reinterpret_cast<uint32_t*>(g_lds_cbc));   // Te0/Te2 copies at LDS 0
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.n) return;
    const uint32_t s = gld(r.session, i);
    if (s >= r.nsessions) {                             // skipped: no row, no iv, no data, no number
        gst(r.wire_len, i, 0u);
        return;
    }
    const CbcKeyDev* key = tab + s;
    const uint64_t q = gld(seq, i);
    if (r.seq_out) gst(r.seq_out, i, q);
    seal_record<NR, H, ETM>(key, q, i, r);
}

template <int NR, class H, bool ETM>
__global__ __launch_bounds__(kCbcThreads) void cbctab_open(const CbcKeyDev* __restrict__ tab,
                                                           tg_cbc_session_records r,
                                                           const uint64_t* __restrict__ seq) {
    stage_td(g_lds_cbc);
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.n) return;
    const uint32_t s = gld(r.session, i);
    if (s >= r.nsessions) {                             // skipped: no row, no wire, no number
        gst(r.status, i, (uint8_t)TG_REC_BAD_SESSION);
        gst(r.data_len, i, 0u);
        gst(r.ctype, i, (uint8_t)0);
        return;
    }
    const CbcKeyDev* key = tab + s;
    const uint64_t q = gld(seq, i);
    if (r.seq_out) gst(r.seq_out, i, q);
    open_record<NR, H, ETM>(key, q, i, r);
}

template <int NR, class H, bool ETM>
int launch2(const CbcKeyDev* tab, const tg_cbc_session_records& r, const uint64_t* seq, bool open,
            hipStream_t s) {
    const unsigned blocks = (unsigned)((r.n + kCbcThreads - 1) / kCbcThreads);   // n < 2^32
    if (open) {
        if (lds_attr((const void*)cbctab_open<NR, H, ETM>, (int)kOpenLds)) return fail(TG_EHIP, "LDS attribute");
        hipLaunchKernelGGL((cbctab_open<NR, H, ETM>), dim3(blocks), dim3(kCbcThreads), kOpenLds, s, tab, r, seq);
    } else {
        if (lds_attr((const void*)cbctab_seal<NR, H, ETM>, (int)kSealLds)) return fail(TG_EHIP, "LDS attribute");
        hipLaunchKernelGGL((cbctab_seal<NR, H, ETM>), dim3(blocks), dim3(kCbcThreads), kSealLds, s, tab, r, seq);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TG_OK : fail(TG_EHIP, "cbc table kernel launch: %s", hipGetErrorString(e));
}

template <int NR, class H>
int launch1(const CbcKeyDev* tab, const tg_cbc_session_records& r, const uint64_t* seq, bool open,
            hipStream_t s) {
    return r.etm ? launch2<NR, H, true>(tab, r, seq, open, s) : launch2<NR, H, false>(tab, r, seq, open, s);
}

template <int NR>
int launch0(int mac, const CbcKeyDev* tab, const tg_cbc_session_records& r, const uint64_t* seq, bool open,
            hipStream_t s) {
    switch (mac) {
        case TG_MAC_SHA1: return launch1<NR, Sha1>(tab, r, seq, open, s);
        case TG_MAC_SHA256: return launch1<NR, Sha256>(tab, r, seq, open, s);
        default: return launch1<NR, Sha384>(tab, r, seq, open, s);
    }
}

int cbc_session_records(tg_cbc_key* k, const tg_cbc_session_records* r, void* stream, bool open) {
    // argument errors first, before any HIP call; those of the struct alone
    // are reported whatever the key is (the order of tg_cbc_records, then
    // that of tg_session_records)
    if (!r) return fail(TG_EINVAL, "null tg_cbc_session_records");
    if (r->version != TG_TLS11 && r->version != TG_TLS12)
        return fail(TG_EINVAL, "version 0x%04x is neither TG_TLS11 nor TG_TLS12", r->version);
    if (r->etm > 1) return fail(TG_EINVAL, "etm must be 0 or 1, got %u", r->etm);
    if (!open && !r->iv) return fail(TG_EINVAL, "seal needs iv (16 bytes per record)");
    if ((r->seq != nullptr) == (r->seq_next != nullptr))
        return fail(TG_EINVAL, "exactly one of seq (explicit numbers) and seq_next (per-session "
                    "counters) must be given, got %s", r->seq ? "both" : "neither");
    if (r->n > 0xfffffffeull) return fail(TG_EINVAL, "at most 2^32 - 2 records per call");
    if (r->n && !r->session) return fail(TG_EINVAL, "null session (one index per record)");
    if (!k) return fail(TG_EINVAL, "null key");
    if (r->nsessions != k->nkeys)
        return fail(TG_EINVAL, "nsessions (%llu) must equal the key handle's nkeys (%llu)",
                    (unsigned long long)r->nsessions, (unsigned long long)k->nkeys);
    if (r->n == 0) return TG_OK;
    if (!r->data || !r->data_off || !r->data_len || !r->ctype || !r->wire || !r->wire_off ||
        !r->wire_len)
        return fail(TG_EINVAL, "null device array");
    if (open && !r->status) return fail(TG_EINVAL, "open needs status");
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != k->device) HIP_TRY(hipSetDevice(k->device));
    hipStream_t s = static_cast<hipStream_t>(stream);

    // counter mode: the rank pass (sessions.hip) numbers the records into
    // per-call scratch and advances the counters, all on the stream
    Scratch scratch(s);
    const uint64_t* seq = r->seq;
    if (r->seq_next) {
        int rc;
        size_t rank_bytes = 0;
        if ((rc = tg_session_rank(nullptr, r->n, r->nsessions, nullptr, nullptr, nullptr, &rank_bytes, s)))
            return fail(rc, "rank pass sizing failed");
        if (scratch.alloc(align_up(r->n * sizeof(uint64_t), 256) + rank_bytes))
            return fail(TG_EHIP, "scratch allocation failed");
        uint64_t* ranked = scratch.take<uint64_t>(r->n * sizeof(uint64_t), 256);
        if ((rc = tg_session_rank(r->session, r->n, r->nsessions, r->seq_next, ranked,
                                  scratch.take<uint8_t>(rank_bytes, 256), &rank_bytes, s)))
            return fail(rc, "rank pass launch failed");
        seq = ranked;
    }
    const int rc = k->rounds == 10 ? launch0<10>(k->mac, k->dev_key, *r, seq, open, s)
                                   : launch0<14>(k->mac, k->dev_key, *r, seq, open, s);
    // the scratch goes back behind the launch
    return scratch.release() && !rc ? fail(TG_EHIP, "scratch release failed") : rc;
}

}  // namespace
}  // namespace tg

extern "C" {

int tg_cbc_seal_session_records(tg_cbc_key* k, const tg_cbc_session_records* r, void* stream) {
    return tg::cbc_session_records(k, r, stream, false);
}

int tg_cbc_open_session_records(tg_cbc_key* k, const tg_cbc_session_records* r, void* stream) {
    return tg::cbc_session_records(k, r, stream, true);
}

}  // extern "C"
