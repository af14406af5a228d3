// cbc_record.h -- HMAC over a TLS record and the receive-side verdicts of
// the AES-CBC + HMAC suites, for one record, as plain C++ that the device
// kernels (aes_cbc.hip) and a host program (tests/native/
// cbc_verdict_check.cpp) both compile: __host__ __device__, no LDS, no
// builtins.  Memory is read through a policy class ``Mem`` (the device reads
// global memory explicitly, the host copies bytes):
//   Mem::ld16(p)     16 bytes at any alignment as four LE words
//   Mem::ldn(p, n)   n < 16 bytes, zero-padded
//   Mem::ld4(p)      4 bytes, LE
//   Mem::ld1(p)      1 byte
//
// hmac_record is calculateMAC (tlslite/recordlayer.py:463-474) with the
// connection's keyed HMAC: the message is
//   be64(seq) || type || version(2) || be16(len) || bytes[0, len)
// and the key enters as the two midstates of the ipad / opad block.  It is
// written for the receive side of MAC-then-encrypt, where ``len`` is secret:
// the caller fixes the number of compression calls (``nblocks``, from the
// longest message the record could hold) and the bytes that may be read
// (``avail``); the message's end, its 0x80 byte, the bit length and the block
// whose state is the digest are all selected with masks.  The send side and
// encrypt-then-MAC call the same code with nblocks = the message's own count.
//
// mte_verdict is ct_check_cbc_mac_and_pad (tlslite/utils/constanttime.py:
// 102-204) for TLS 1.1 / 1.2 with the same verdict on every input, without
// its "every possible MAC" loop: one MAC, over mac_start bytes, compared at
// mac_start -- the only position where that loop's mask is non-zero.  Its
// cost (compression calls, bytes read) depends on the record's length and the
// hash alone, never on the decrypted bytes.
#pragma once
#include "sha.h"

namespace tg {
namespace cbc {

struct W4 {
    uint32_t x, y, z, w;
};

// HMAC key as the hash states after the ipad and the opad block.
struct Mid {
    uint64_t inner[8];
    uint64_t outer[8];
};

TG_HDI uint32_t bswap(uint32_t v) {
    return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
}

// Compression calls of the inner hash for a message of 13 + len bytes.
template <class H>
TG_HDI uint32_t hmac_blocks(uint32_t len) {
    return (13u + len + (uint32_t)H::kLenBytes) / (uint32_t)H::kBlock + 1u;
}

// 16 message bytes at message offset mo (a multiple of 16) as LE words: the
// 13-byte header (LE words h0..h3, byte 13.. zero), then the data.  Reads
// only data[0, avail).
template <class Mem>
TG_HDI W4 msg_chunk(const W4& hdr, const uint8_t* data, uint32_t avail, uint32_t mo) {
    if (mo == 0) {
        const uint32_t n = avail < 3u ? avail : 3u;
        const W4 d = Mem::ldn(data, n);
        return W4{hdr.x, hdr.y, hdr.z, hdr.w | (d.x << 8)};
    }
    const uint32_t off = mo - 13u;
    if (off + 16u <= avail) return Mem::ld16(data + off);
    if (off < avail) return Mem::ldn(data + off, avail - off);
    return W4{0, 0, 0, 0};
}

// Big-endian message word at message offset o of a message that ends at
// ``end`` (0x80 follows it): v holds the four bytes in memory order (LE).
TG_HDI uint32_t msg_word(uint32_t v, uint32_t o, uint32_t end) {
    const uint32_t be = bswap(v);
    const int32_t n = (int32_t)(end - o);                  // bytes of this word inside the message
    const uint32_t nn = n < 0 ? 0u : (n > 4 ? 4u : (uint32_t)n);
    const uint32_t keep = (uint32_t)~(0xffffffffull >> (8u * nn));
    const uint32_t term = (uint32_t)n < 4u ? (0x80000000u >> (8u * ((uint32_t)n & 3u))) : 0u;
    return (be & keep) | term;
}

// dig: the HMAC as big-endian 32-bit words (H::kHash / 4 of them).
template <class H, class Mem>
TG_HDI void hmac_record(const Mid& mid, uint64_t seq, uint32_t type, uint32_t version,
                              const uint8_t* data, uint32_t avail, uint32_t len, uint32_t nblocks,
                              uint32_t dig[12]) {
    using W = typename H::word;
    constexpr uint32_t B = H::kBlock, NW = B / 4;
    const uint32_t end = 13u + len;
    const uint32_t last = (end + (uint32_t)H::kLenBytes) / B;   // block that carries the length
    const uint32_t bits = (B + end) * 8u;
    const uint32_t s_hi = (uint32_t)(seq >> 32), s_lo = (uint32_t)seq;
    W4 hdr;
    hdr.x = bswap(s_hi);
    hdr.y = bswap(s_lo);
    hdr.z = (type & 0xffu) | ((version >> 8) & 0xffu) << 8 | (version & 0xffu) << 16 |
            ((len >> 8) & 0xffu) << 24;
    hdr.w = len & 0xffu;
    W st[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        st[k] = (W)mid.inner[k];
        out[k] = 0;
    }
    for (uint32_t b = 0; b < nblocks; ++b) {
        uint32_t m32[NW];
#pragma unroll
        for (uint32_t c = 0; c < B / 16; ++c) {
            const uint32_t mo = b * B + 16u * c;
            const W4 v = msg_chunk<Mem>(hdr, data, avail, mo);
            m32[4 * c] = msg_word(v.x, mo, end);
            m32[4 * c + 1] = msg_word(v.y, mo + 4, end);
            m32[4 * c + 2] = msg_word(v.z, mo + 8, end);
            m32[4 * c + 3] = msg_word(v.w, mo + 12, end);
        }
        const uint32_t is_last = b == last ? 0xffffffffu : 0u;
        m32[NW - 1] |= bits & is_last;
        W m[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if constexpr (sizeof(W) == 4) {
                m[k] = (W)m32[k];
            } else {
                m[k] = (W)(((uint64_t)m32[2 * k] << 32) | m32[2 * k + 1]);
            }
        }
        H::compress(st, m);
        const W sel = (W)0 - (W)(is_last & 1u);
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = (out[k] & ~sel) | (st[k] & sel);
    }
    // outer: H((K ^ opad) || inner digest), one padded block
    W m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = k < H::kStateOut ? out[k] : (W)0;
    m[H::kStateOut] = (W)1 << (8 * sizeof(W) - 1);         // 0x80 terminator
    m[15] = (W)((B + (uint32_t)H::kHash) * 8u);
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = (W)mid.outer[k];
    H::compress(st, m);
#pragma unroll
    for (int k = 0; k < 12; ++k) dig[k] = 0;
#pragma unroll
    for (int k = 0; k < H::kStateOut; ++k) {
        if constexpr (sizeof(W) == 4) {
            dig[k] = (uint32_t)st[k];
        } else {
            dig[2 * k] = (uint32_t)((uint64_t)st[k] >> 32);
            dig[2 * k + 1] = (uint32_t)st[k];
        }
    }
}

// Non-zero when the H::kHash bytes at p differ from the digest; no early exit.
template <class H, class Mem>
TG_HDI uint32_t mac_differs(const uint8_t* p, const uint32_t dig[12]) {
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < H::kHash / 4; ++k) diff |= bswap(Mem::ld4(p + 4 * k)) ^ dig[k];
    return diff;
}

// TLS >= 1.0 padding check over the last min(256, n) bytes of p[0, n), n a
// multiple of 16: non-zero when a byte at or after pad_start differs from pad
// (constanttime.py:159-164).  Reads the same bytes whatever pad_start is.
template <class Mem>
TG_HDI uint32_t pad_differs(const uint8_t* p, uint32_t n, uint32_t pad, uint32_t pad_start) {
    const uint32_t want = pad * 0x01010101u;
    uint32_t bad = 0;
    for (uint32_t c = n > 256u ? n - 256u : 0u; c < n; c += 16u) {
        const W4 v = Mem::ld16(p + c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            // bytes of this word at or after pad_start: the top ``in`` bytes (LE)
            const int32_t d = (int32_t)(c + 4u * k + 4u - pad_start);
            const uint32_t in = d < 0 ? 0u : (d > 4 ? 4u : (uint32_t)d);
            const uint32_t mask = (uint32_t)(0xffffffffull << (8u * (4u - in)));
            bad |= (w[k] ^ want) & mask;
        }
    }
    return bad;
}

// The per-record status codes of include/tlsgpu.h (TG_REC_*) that this path
// reports; this header stands alone, aes_cbc.hip asserts they agree.
constexpr uint32_t kRecOk = 0, kRecBadMac = 1, kRecOverflow = 7, kRecDecryptFailed = 9;

// What is decided from public lengths before a MAC-then-encrypt record is
// decrypted (RecordSocket.recv :219-220, _decryptThenMAC :691-692,
// constanttime.py:138-139): kRecOk means "decrypt body - 16 bytes and ask
// mte_verdict".  hlen: the header's length field, body: the bytes behind it.
TG_HDI uint32_t mte_public_status(uint32_t hash_len, uint32_t hlen, uint32_t body, uint32_t limit) {
    if (hlen > limit + 2048u || body > limit + 2048u) return kRecOverflow;
    if (body & 15u) return kRecDecryptFailed;
    const uint32_t n = body >= 16u ? body - 16u : 0u;       // behind the IV block (:694-695)
    if (n < hash_len + 1u) return kRecBadMac;
    return kRecOk;
}

// The status after the verdict: recvRecord's plaintext limit (:980-981).
TG_HDI uint32_t final_status(uint32_t bad, uint32_t len, uint32_t limit) {
    return bad ? kRecBadMac : (len > limit ? kRecOverflow : kRecOk);
}

// The HMAC key as midstates: the hash state after (key, zero-padded) ^ 0x36
// and after (key, zero-padded) ^ 0x5c.  keylen <= H::kBlock.
template <class H>
TG_HDI void hmac_midstates(const uint8_t* key, uint32_t keylen, Mid* mid) {
    using W = typename H::word;
    for (int side = 0; side < 2; ++side) {
        const uint8_t fill = side ? 0x5c : 0x36;
        W m[16], st[8];
        for (int k = 0; k < 16; ++k) {
            W v = 0;
            for (uint32_t b = 0; b < sizeof(W); ++b) {
                const uint32_t at = (uint32_t)k * sizeof(W) + b;
                v = (W)((v << 8) | (uint8_t)((at < keylen ? key[at] : 0) ^ fill));
            }
            m[k] = v;
        }
        H::init(st);
        H::compress(st, m);
        for (int k = 0; k < 8; ++k) (side ? mid->outer : mid->inner)[k] = (uint64_t)st[k];
        for (int k = 0; k < 16; ++k) m[k] = 0;
    }
}

// MAC-then-encrypt: p[0, n) is the decrypted record after its IV block, n a
// multiple of 16.  Returns 0 when padding and MAC are good (then *len is the
// plaintext length), non-zero for TLSBadRecordMAC.
template <class H, class Mem>
TG_HDI uint32_t mte_verdict(const Mid& mid, uint64_t seq, uint32_t type, uint32_t version,
                                  const uint8_t* p, uint32_t n, uint32_t* len) {
    *len = 0;
    if ((uint32_t)H::kHash + 1u > n) return 1;             // n is public (constanttime.py:138)
    const uint32_t pad = Mem::ld1(p + n - 1);
    const uint32_t pad_start = n >= pad + 1u ? n - pad - 1u : 0u;
    const uint32_t mac_start = pad_start >= (uint32_t)H::kHash ? pad_start - (uint32_t)H::kHash : 0u;
    uint32_t bad = pad_differs<Mem>(p, n, pad, pad_start);
    uint32_t dig[12];
    hmac_record<H, Mem>(mid, seq, type, version, p, n, mac_start,
                        hmac_blocks<H>(n - (uint32_t)H::kHash - 1u), dig);
    bad |= mac_differs<H, Mem>(p + mac_start, dig);
    *len = mac_start;
    return bad;
}

// Encrypt-then-MAC, after the MAC was found good: the padding of the
// decrypted p[0, n), n > 0 (recordlayer.py:759-776).
template <class Mem>
TG_HDI uint32_t etm_padding(const uint8_t* p, uint32_t n, uint32_t* len) {
    *len = 0;
    const uint32_t pad = Mem::ld1(p + n - 1);
    if (pad + 1u > n) return 1;
    if (pad_differs<Mem>(p, n, pad, n - pad - 1u)) return 1;
    *len = n - pad - 1u;
    return 0;
}

}  // namespace cbc
}  // namespace tg
