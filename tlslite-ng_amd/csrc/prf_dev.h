// prf_dev.h -- what the TLS key-derivation translation units share (tls12.hip:
// the TLS 1.2 PRF and its installs; tls10.hip: the TLS 1.0 / 1.1 PRF and its
// install): HMAC with the key as two midstates, the HMAC of a packed message
// template, P_hash into a register window, the CBC table row, and the launch
// and argument checks both files make.  Anonymous namespace, as keysetup_dev.h:
// each translation unit has its own copy.
//
// Byte order.  A hash H says with H::kBigEndian how its message words, its bit
// length and its digest are laid out (sha.h: big-endian, the length in the
// block's last word; md5.h: little-endian, the length's low word in word 14).
// Everything here that builds a block or reads a digest asks the trait; keys,
// templates and digests are always "words of H", in H's own order.
#pragma once
#include "api.h"
#include "cbc_dev.h"
#include "keysetup_dev.h"
#include "runtime.h"

namespace tg {
namespace {

// ---- HMAC with the key as midstates ----------------------------------------
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

// st = HMAC over a packed template of nb blocks (t: its word 0 for this lane,
// words n apart, in H's byte order).  SPLICE: the digest a replaces the hole at
// its front.
template <class H, bool SPLICE>
__device__ __forceinline__ void hm_tmpl(const Hm<H>& h, const uint32_t* __restrict__ t, uint64_t n, uint32_t nb,
                                        const typename H::word a[8], typename H::word st[8]) {
    using W = typename H::word;
    W hole[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        hole[k] = a[k];
        st[k] = h.in[k];
    }
    for (uint32_t b = 0; b < nb; ++b) {   // uniform: nb comes from the lengths
        W blk[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if constexpr (sizeof(W) == 4) {
                blk[k] = t[(uint64_t)(16 * b + k) * n];
            } else {
                blk[k] = ((uint64_t)t[(uint64_t)(32 * b + 2 * k) * n] << 32) | t[(uint64_t)(32 * b + 2 * k + 1) * n];
            }
        }
        if (SPLICE && b == 0) {
#pragma unroll
            for (int k = 0; k < H::kStateOut; ++k) blk[k] = hole[k];
        }
        H::compress(st, blk);
    }
    hm_outer<H>(h, st);
}

// ---- P_hash into registers ---------------------------------------------------
// The first NB digests of P_hash (mathtls.py:679-698) under the keyed h, as
// big-endian 32-bit words of the output's bytes whatever H's order is.  t1 /
// t2: this lane's word 0 of the templates of A(0) and of A(i) || A(0).
// The window moves down one digest per block (compile-time indices inside a
// loop that is not unrolled); after NB rounds digest 0 is at kb[0].
// (key_block of tls12.hip is this loop with the master secret's load in front;
// it keeps its own text so that the TLS 1.2 kernels stay instruction for
// instruction what they were.)
template <class H, int NB>
__device__ __forceinline__ void p_hash_words(const Hm<H>& h, const uint32_t* __restrict__ t1, uint32_t nb1,
                                             const uint32_t* __restrict__ t2, uint32_t nb2, uint64_t n,
                                             uint32_t kb[NB * (H::kHash / 4)]) {
    using W = typename H::word;
    constexpr int HW = H::kHash / 4;
    W a[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = 0;
#pragma unroll
    for (int k = 0; k < NB * HW; ++k) kb[k] = 0;
    hm_tmpl<H, false>(h, t1, n, nb1, a, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = o[k];
#pragma unroll 1
    for (int b = 0; b < NB; ++b) {
        hm_tmpl<H, true>(h, t2, n, nb2, a, o);
        uint32_t d[12];
        digest_words<H>(o, d);
#pragma unroll
        for (int k = 0; k < (NB - 1) * HW; ++k) kb[k] = kb[k + HW];
#pragma unroll
        for (int k = 0; k < HW; ++k) {
            if constexpr (H::kBigEndian) kb[(NB - 1) * HW + k] = d[k];
            else kb[(NB - 1) * HW + k] = bswap32(d[k]);
        }
        if (b + 1 < NB) {
            hm_digest<H>(h, a, o);
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] = o[k];
        }
    }
}

// ---- CBC rows ------------------------------------------------------------------
// InvMixColumns of one column, the four bytes at once; inv_mix_column of
// cbc_dev.h (the host's) is the definition.
constexpr uint32_t xtime_x4(uint32_t w) { return ((w & 0x7f7f7f7fu) << 1) ^ (((w >> 7) & 0x01010101u) * 0x1bu); }
constexpr uint32_t ror32(uint32_t w, int n) { return (w >> n) | (w << (32 - n)); }
constexpr uint32_t inv_mix_x4(uint32_t w) {
    const uint32_t x2 = xtime_x4(w), x4 = xtime_x4(x2), x8 = xtime_x4(x4);
    const uint32_t m9 = x8 ^ w, mb = m9 ^ x2, md = m9 ^ x4, me = x8 ^ x4 ^ x2;
    // b_i = 0e a_i ^ 0b a_(i+1) ^ 0d a_(i+2) ^ 09 a_(i+3), byte i of a LE word
    return me ^ ror32(mb, 8) ^ ror32(md, 16) ^ ror32(m9, 24);
}
static_assert(inv_mix_x4(0x00000001u) == inv_mix_column(0x00000001u), "InvMixColumns");
static_assert(inv_mix_x4(0x8f3c21e7u) == inv_mix_column(0x8f3c21e7u), "InvMixColumns");
static_assert(inv_mix_x4(0xffa05b80u) == inv_mix_column(0xffa05b80u), "InvMixColumns");
static_assert(inv_mix_x4(0x1b9d4fc6u) == inv_mix_column(0x1b9d4fc6u), "InvMixColumns");

// Every byte of row o, as build_row (aes_cbc.hip) builds it on the host.
// rk[0 .. NK): the cipher key as LE words; m: the MAC key as big-endian words,
// zero-padded to one block of HM.
template <int NK, class HM>
__device__ __forceinline__ void store_cbc_row(const uint8_t* sb, uint32_t rk[60], const typename HM::word m[16],
                                              CbcKeyDev* o, uint32_t mac) {
    constexpr int NR = NK + 6;
    expand_words<NK>(sb, rk);
#pragma unroll
    for (int k = 0; k < 60; ++k) o->ek[k] = rk[k];
#pragma unroll
    for (int r = 0; r <= NR; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t w = rk[4 * (NR - r) + c];
            o->dk[4 * r + c] = (r == 0 || r == NR) ? w : inv_mix_x4(w);
        }
#pragma unroll
    for (int k = 4 * (NR + 1); k < 60; ++k) o->dk[k] = 0;
    Hm<HM> h;
    hm_key<HM>(m, h);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        o->mid.inner[k] = (uint64_t)h.in[k];
        o->mid.outer[k] = (uint64_t)h.out[k];
    }
    o->rounds = NR;
    o->mac = mac;
    o->pad[0] = 0;
    o->pad[1] = 0;
}

// ---- launches and the checks of a tg_tls12_install ------------------------------
inline bool launched() { return hipGetLastError() == hipSuccess; }

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

constexpr uint64_t kMaxSessions = 1ull << 31;   // grids of every kernel stay below 2^31 blocks

const uint8_t kKeyExpansion[] = "key expansion";

// The struct's own errors, whatever the key is (tg_sessions_rekey's order).
// hashed: hashlen is read (TLS 1.2); aead: fixed_iv_len and iv_table are.
inline int install_struct_error(const tg_tls12_install* r, bool aead, bool hashed = true) {
    if (!r) return fail(TG_EINVAL, "null tg_tls12_install");
    if (hashed && r->hashlen != 32 && r->hashlen != 48)
        return fail(TG_EINVAL, "hashlen must be 32 or 48, got %u", r->hashlen);
    if (r->side != TG_TLS12_CLIENT_WRITE && r->side != TG_TLS12_SERVER_WRITE)
        return fail(TG_EINVAL, "side %u is neither TG_TLS12_CLIENT_WRITE nor TG_TLS12_SERVER_WRITE", r->side);
    if (aead && r->fixed_iv_len != 4 && r->fixed_iv_len != 12)
        return fail(TG_EINVAL, "fixed_iv_len must be 4 or 12, got %u", r->fixed_iv_len);
    if (aead && !r->iv_table) return fail(TG_EINVAL, "null iv_table");
    if (!r->master_secrets || !r->client_random || !r->server_random)
        return fail(TG_EINVAL, "null master_secrets, client_random or server_random");
    return TG_OK;
}

inline int install_count_error(const tg_tls12_install* r, uint64_t nkeys) {
    if (r->nsessions != nkeys)
        return fail(TG_EINVAL, "nsessions (%llu) must equal the key handle's nkeys (%llu)",
                    (unsigned long long)r->nsessions, (unsigned long long)nkeys);
    if (r->n > nkeys)
        return fail(TG_EINVAL, "n (%llu) is above the key handle's nkeys (%llu)", (unsigned long long)r->n,
                    (unsigned long long)nkeys);
    if (r->n > kMaxSessions) return fail(TG_EINVAL, "n must be at most 2^31");
    return TG_OK;
}

}  // namespace
}  // namespace tg
