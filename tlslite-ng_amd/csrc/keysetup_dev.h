// keysetup_dev.h -- device functions every key-setup translation unit shares
// (keysetup.hip: TLS 1.3 derivation and rekey; tls12.hip and tls10.hip through
// prf_dev.h: the TLS 1.0 - 1.2 PRFs, their fused installs and the CBC rows;
// tls13.hip: the TLS 1.3 key schedule).  The one text of each primitive:
//   unaligned word access, the digest as 32-bit words and its stores
//     (store_words, store_digest, store_digest_bytes);
//   an HMAC key from bytes (key_from_bytes: run-time length) or from a row
//     (key_from_row: compile-time length, word loads);
//   HMAC with the key as two midstates (Hm, hm_key, digest_block, hm_outer,
//     hm_digest), in the byte order H::kBigEndian states;
//   HKDF's T(1) over a shared message (hkdf_t1), on that HMAC;
//   the AES key schedule, the per-layout entry store and H = E_K(0).
// Everything sits in an anonymous namespace: each translation unit has its
// own copy, kernels are launched from the file that defines them.
#pragma once
#include "aes_bs8.h"
#include "common.h"
#include "sha.h"

namespace tg {
namespace {

// ------------------------------------------------- unaligned global words --
typedef uint32_t u32_u1 __attribute__((aligned(1)));

__device__ __forceinline__ uint32_t load_u32u(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const __attribute__((address_space(1))) u32_u1*)p;
#else
    return 0;
#endif
}
__device__ __forceinline__ void store_u32u(uint8_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(__attribute__((address_space(1))) u32_u1*)p = v;
#endif
}

// ---------------------------------------------------------- digests out --
// The digest as big-endian 32-bit words of its bytes.
template <class H>
__device__ __forceinline__ void digest_words(const typename H::word st[8], uint32_t d[12]) {
    if constexpr (sizeof(typename H::word) == 4) {
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = st[k];
#pragma unroll
        for (int k = 8; k < 12; ++k) d[k] = 0;
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            d[2 * k] = (uint32_t)(st[k] >> 32);
            d[2 * k + 1] = (uint32_t)st[k];
        }
    }
}

// N big-endian words as their 4 N bytes, any alignment.
template <int N>
__device__ __forceinline__ void store_words(const uint32_t* d, uint8_t* to) {
#pragma unroll
    for (int k = 0; k < N; ++k) store_u32u(to + 4 * k, bswap32(d[k]));
}

// The whole digest (of a big-endian H), any alignment.
template <class H>
__device__ __forceinline__ void store_digest(const typename H::word st[8], uint8_t* to) {
    uint32_t d[12];
    digest_words<H>(st, d);
    store_words<H::kHash / 4>(d, to);
}

// The digest's first min(outlen, hash length) bytes, one by one.
template <class H>
__device__ __forceinline__ void store_digest_bytes(const typename H::word st[8], uint8_t* to, uint32_t outlen) {
    constexpr int WB = sizeof(typename H::word);
    const gptr op = (gptr)to;
#pragma unroll
    for (int k = 0; k < H::kHash; ++k)
        if ((uint32_t)k < outlen) op[k] = (uint8_t)(st[k / WB] >> (8 * (WB - 1 - (k % WB))));
}

// ------------------------------------------------------ HMAC keys loaded --
// An HMAC key is sixteen words of H in H's byte order (H::kBigEndian),
// zero-padded to one hash block.
// key_from_bytes: len <= block bytes at p, a run-time length, byte loads.
template <class H>
__device__ __forceinline__ void key_from_bytes(const uint8_t* p, uint32_t len, typename H::word key[16]) {
    using W = typename H::word;
    constexpr int WB = sizeof(W);
    const gptr_c g = (gptr_c)p;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        W v = 0;
#pragma unroll
        for (int b = 0; b < WB; ++b) {
            const uint32_t at = (uint32_t)(k * WB + b);
            uint32_t byte = 0;
            if (at < len) byte = g[at];
            if constexpr (H::kBigEndian) v = (W)((v << 8) | byte);
            else v |= (W)byte << (8 * b);
        }
        key[k] = v;
    }
}

// key_from_row: BYTES bytes at row (any alignment), word loads.  NULLABLE: a
// NULL row stands for zeros (the TLS 1.3 schedule's absent salt and PSK); the
// check sits on every load, so the callers whose row cannot be NULL leave it out.
template <class H, int BYTES, bool NULLABLE = false>
__device__ __forceinline__ void key_from_row(const uint8_t* row, typename H::word key[16]) {
    using W = typename H::word;
    constexpr int WB = sizeof(W);
    static_assert(BYTES % WB == 0 && BYTES <= 16 * WB, "whole words of one block");
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k * WB >= BYTES || (NULLABLE && !row)) {
            key[k] = W(0);
        } else if constexpr (!H::kBigEndian) {
            key[k] = load_u32u(row + 4 * k);
        } else if constexpr (WB == 4) {
            key[k] = bswap32(load_u32u(row + 4 * k));
        } else {
            key[k] = ((uint64_t)bswap32(load_u32u(row + 8 * k)) << 32) | bswap32(load_u32u(row + 8 * k + 4));
        }
    }
}

// ---------------------------------------- HMAC with the key as midstates --
template <class H>
struct Hm {
    typename H::word in[8], out[8];
};

// key: the HMAC key as words of H, zero-padded to one hash block.
template <class H>
__device__ __forceinline__ void hm_key(const typename H::word key[16], Hm<H>& h) {
    using W = typename H::word;
    const W ipad = (W)0x3636363636363636ull, opad = (W)0x5c5c5c5c5c5c5c5cull;
    W blk[16];
    H::init(h.in);
#pragma unroll
    for (int k = 0; k < 16; ++k) blk[k] = key[k] ^ ipad;
    H::compress(h.in, blk);
    H::init(h.out);
#pragma unroll
    for (int k = 0; k < 16; ++k) blk[k] = key[k] ^ opad;
    H::compress(h.out, blk);
}

// One digest as the whole message behind a key block: its padded block.
template <class H>
__device__ __forceinline__ void digest_block(const typename H::word d[8], typename H::word blk[16]) {
    using W = typename H::word;
    constexpr int dw = H::kStateOut;
#pragma unroll
    for (int k = 0; k < 16; ++k) blk[k] = k < dw ? d[k] : W(0);
    if constexpr (H::kBigEndian) {
        blk[dw] = (W)1 << (8 * sizeof(W) - 1);                  // 0x80 terminator
        blk[15] = (W)((H::kBlock + H::kHash) * 8);              // bit length of block + digest
    } else {
        blk[dw] = (W)0x80;
        blk[14] = (W)((H::kBlock + H::kHash) * 8);              // its low word; word 15 stays 0
    }
}

// st: the inner digest on entry, the HMAC on return.
template <class H>
__device__ __forceinline__ void hm_outer(const Hm<H>& h, typename H::word st[8]) {
    typename H::word blk[16];
    digest_block<H>(st, blk);
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = h.out[k];
    H::compress(st, blk);
}

// st = HMAC(a), a one digest: A(i + 1) from A(i).
template <class H>
__device__ __forceinline__ void hm_digest(const Hm<H>& h, const typename H::word a[8], typename H::word st[8]) {
    typename H::word blk[16];
    digest_block<H>(a, blk);
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = h.in[k];
    H::compress(st, blk);
    hm_outer<H>(h, st);
}

// ------------------------------------------------------- HKDF-Expand T(1) --
// HMAC(secret, info || 0x01): HKDF_expand's first block T(1)
// (cryptomath.py:146-153), which is all of it for outlen <= hash length.
// msg: info || 0x01 SHA-padded, the same for every session (keysetup.hip:
// hkdf_kernel, rekey_kernel; tls13.hip: the steps whose HkdfLabel is shared).
// key: the secret as an HMAC key; st receives the digest words.
template <class H>
__device__ __forceinline__ void hkdf_t1(const tg::HkdfMsg& msg, const typename H::word key[16],
                                        typename H::word st[8]) {
    using W = typename H::word;
    Hm<H> h;
    hm_key<H>(key, h);
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = h.in[k];
    for (uint32_t b = 0; b < msg.nblocks; ++b) {   // uniform message blocks
        W blk[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if constexpr (sizeof(W) == 4) {
                blk[k] = msg.words[16 * b + k];
            } else {
                blk[k] = ((uint64_t)msg.words[32 * b + 2 * k] << 32) | msg.words[32 * b + 2 * k + 1];
            }
        }
        H::compress(st, blk);
    }
    hm_outer<H>(h, st);
}

// ------------------------------------------------------- AES key schedule --
constexpr uint8_t xtime8(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }

struct SboxTable {
    uint8_t s[256];
};

constexpr SboxTable make_sbox() {
    uint8_t exp[256] = {};
    uint8_t log[256] = {};
    uint8_t x = 1;
    for (int i = 0; i < 255; ++i) {
        exp[i] = x;
        log[x] = (uint8_t)i;
        x = (uint8_t)(x ^ xtime8(x));
    }
    SboxTable t = {};
    for (int v = 0; v < 256; ++v) {
        uint8_t inv = v ? exp[(255 - log[v]) % 255] : 0;
        uint8_t s = inv, r = inv;
        for (int k = 0; k < 4; ++k) {
            r = (uint8_t)((r << 1) | (r >> 7));
            s = (uint8_t)(s ^ r);
        }
        t.s[v] = (uint8_t)(s ^ 0x63);
    }
    return t;
}

__constant__ SboxTable c_sbox = make_sbox();

__device__ __forceinline__ uint32_t sub_word(const uint8_t* sb, uint32_t w) {
    return (uint32_t)sb[w & 0xff] | ((uint32_t)sb[(w >> 8) & 0xff] << 8) |
           ((uint32_t)sb[(w >> 16) & 0xff] << 16) | ((uint32_t)sb[w >> 24] << 24);
}

// FIPS-197 key expansion (rijndael.py:922-993); words are LE words of the
// key-schedule bytes (the layout every AES kernel reads).
// expand_words: rk[0 .. NK) hold the key already.
template <int NK>
__device__ __forceinline__ void expand_words(const uint8_t* sb, uint32_t rk[60]) {
    constexpr int NR = NK + 6, TOTAL = 4 * (NR + 1);
    uint32_t rcon = 1;
#pragma unroll
    for (int k = NK; k < TOTAL; ++k) {
        uint32_t t = rk[k - 1];
        if (k % NK == 0) {
            t = sub_word(sb, (t >> 8) | (t << 24)) ^ rcon;   // SubWord(RotWord(t)) ^ Rcon
            rcon = xtime8((uint8_t)rcon);
        } else if (NK > 6 && k % NK == 4) {
            t = sub_word(sb, t);
        }
        rk[k] = rk[k - NK] ^ t;
    }
#pragma unroll
    for (int k = TOTAL; k < 60; ++k) rk[k] = 0;
}

template <int NK>
__device__ __forceinline__ void expand_key(const uint8_t* sb, const uint8_t* key, uint32_t rk[60]) {
#pragma unroll
    for (int k = 0; k < NK; ++k)
        rk[k] = (uint32_t)key[4 * k] | ((uint32_t)key[4 * k + 1] << 8) |
                ((uint32_t)key[4 * k + 2] << 16) | ((uint32_t)key[4 * k + 3] << 24);
    expand_words<NK>(sb, rk);
}

// E_K(0^128) bytewise (SubBytes, ShiftRows, MixColumns) -> H as 4 LE words.
template <int NR>
__device__ __forceinline__ void aes_zero_block(const uint8_t* sb, const uint32_t rk[60], uint32_t h[4]) {
    uint8_t s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = (uint8_t)(rk[k >> 2] >> (8 * (k & 3)));
#pragma unroll
    for (int r = 1; r <= NR; ++r) {
        uint8_t t[16];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int row = 0; row < 4; ++row) t[4 * c + row] = sb[s[4 * ((c + row) & 3) + row]];
        if (r != NR) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                uint8_t* a = t + 4 * c;
                const uint8_t all = (uint8_t)(a[0] ^ a[1] ^ a[2] ^ a[3]), a0 = a[0];
                a[0] = (uint8_t)(a[0] ^ all ^ xtime8((uint8_t)(a[0] ^ a[1])));
                a[1] = (uint8_t)(a[1] ^ all ^ xtime8((uint8_t)(a[1] ^ a[2])));
                a[2] = (uint8_t)(a[2] ^ all ^ xtime8((uint8_t)(a[2] ^ a[3])));
                a[3] = (uint8_t)(a[3] ^ all ^ xtime8((uint8_t)(a[3] ^ a0)));
            }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] = (uint8_t)(t[k] ^ (rk[4 * r + (k >> 2)] >> (8 * (k & 3))));
    }
#pragma unroll
    for (int w = 0; w < 4; ++w)
        h[w] = (uint32_t)s[4 * w] | ((uint32_t)s[4 * w + 1] << 8) | ((uint32_t)s[4 * w + 2] << 16) |
               ((uint32_t)s[4 * w + 3] << 24);
}

// out layouts: 0 = GcmKeyDev (single key), 1 = GcmTableKey[n], 2 = AesKeyDev[n]
// Entry i of ``out`` from its expanded schedule: every byte of the entry is
// written (layout 0: rk, rounds, pad and H parked in ghash[0]; the rest of a
// GcmKeyDev is the launcher's chain).
template <int NK, int LAYOUT>
__device__ __forceinline__ void store_aes_entry(const uint8_t* sb, const uint32_t rk[60], void* out, uint64_t i) {
    constexpr int NR = NK + 6;
    if (LAYOUT == 2) {
        AesKeyDev* o = static_cast<AesKeyDev*>(out) + i;
#pragma unroll
        for (int k = 0; k < 60; ++k) o->rk[k] = rk[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) o->pad[k] = 0;
        return;
    }
    uint32_t h[4];
    aes_zero_block<NR>(sb, rk, h);
    if (LAYOUT == 1) {
        GcmTableKey* o = static_cast<GcmTableKey*>(out) + i;
#pragma unroll
        for (int k = 0; k < 60; ++k) o->rk[k] = rk[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) o->hn[k] = __builtin_bswap32(__builtin_bitreverse32(h[k]));
        return;
    }
    GcmKeyDev* o = static_cast<GcmKeyDev*>(out);   // n == 1
#pragma unroll
    for (int k = 0; k < 60; ++k) o->rk[k] = rk[k];
    o->rounds = NR;
#pragma unroll
    for (int k = 0; k < 3; ++k) o->pad[k] = 0;
    o->ghash[0] = make_uint4(h[0], h[1], h[2], h[3]);   // H parked in entry (0, 0), see keysetup.hip
}

}  // namespace
}  // namespace tg
