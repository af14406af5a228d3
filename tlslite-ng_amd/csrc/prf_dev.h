// prf_dev.h -- what the TLS 1.0 - 1.2 key-derivation translation units share
// (tls12.hip: the TLS 1.2 PRF and its installs; tls10.hip: the TLS 1.0 / 1.1 PRF
// and its install; tls13.hip takes the launch helpers): the HMAC of a packed
// message template, P_hash into a register window, the slices of a key block,
// the CBC table row, the template packer (one word's text for both pack
// kernels, and the host's scratch / pack / launch / release sequence) and the
// argument checks the entry points share.  The HMAC core and the key loads are
// keysetup_dev.h's.  Anonymous namespace, as there: each translation unit has
// its own copy.
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

// ---- HMAC over a packed template (Hm, hm_key, hm_outer: keysetup_dev.h) ------
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

// ---- slices of the key block ---------------------------------------------------
// The key block holds a client's N words at kb[at] and the server's N behind
// them; out gets this side's.  Both sides' words are read as values and one is
// selected: a select of two addresses inside kb would keep the window in memory.
template <int N>
__device__ __forceinline__ void side_words(const uint32_t* kb, int at, bool server, uint32_t* out) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint32_t c = kb[at + k], sv = kb[at + N + k];
        out[k] = server ? sv : c;
    }
}

// A MAC key of HM's digest length, big-endian 32-bit words, as words of HM
// zero-padded to one block (store_cbc_row's m).
template <class HM>
__device__ __forceinline__ void mac_words(const uint32_t mk[HM::kHash / 4], typename HM::word m[16]) {
    constexpr int MW = HM::kHash / 4;
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = 0;
#pragma unroll
    for (int k = 0; k < MW; ++k) {
        if constexpr (sizeof(typename HM::word) == 4) m[k] = mk[k];
        else if (k % 2 == 0) m[k / 2] = ((uint64_t)mk[k] << 32) | mk[k + 1];
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

// ---- launches ---------------------------------------------------------------------
inline bool launched() { return hipGetLastError() == hipSuccess; }

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

constexpr uint64_t kMaxSessions = 1ull << 31;   // grids of every kernel stay below 2^31 blocks

// ---- message templates ----------------------------------------------------------
// What every template of a launch shares: label and seed (public handshake
// values) and where the words go, word w of session i at tmpl[w * n + i].  How
// many templates there are and how long each is is the file's own geometry
// (PrfGeom of tls12.hip, Tls10Geom of tls10.hip).
struct Pack {
    uint32_t label[8];      // LE words of the label's bytes
    uint32_t labellen;
    uint32_t len0, len1;    // the seed is row i of seed0 then row i of seed1
    const uint8_t* seed0;
    const uint8_t* seed1;
    uint64_t n;
    uint32_t* tmpl;
    uint32_t words;         // of all templates of one session
};

// Word wi of session i's template of ``words`` words: a hole of ``hole`` bytes
// (A(i)'s place), label, seed, 0x80, zeros and the bit length behind a key
// block of ``block`` bytes.  le: MD5's order (little-endian words, the length's
// low word last but one); else SHA's (big-endian, the length in the last word).
__device__ __forceinline__ uint32_t pack_word(const Pack& p, uint64_t i, uint32_t wi, uint32_t hole, uint32_t words,
                                              uint32_t block, bool le) {
    const uint32_t s0 = hole + p.labellen, s1 = s0 + p.len0, end = s1 + p.len1;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t at = 4 * wi + b;
        uint32_t byte = 0;
        if (at < hole) {
            byte = 0;
        } else if (at < s0) {
            const uint32_t idx = at - hole;
            uint32_t lw = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) lw = (idx >> 2) == k ? p.label[k] : lw;
            byte = (lw >> (8 * (idx & 3))) & 0xffu;
        } else if (at < s1) {
            byte = ((gptr_c)p.seed0)[(uint64_t)p.len0 * i + (at - s0)];
        } else if (at < end) {
            byte = ((gptr_c)p.seed1)[(uint64_t)p.len1 * i + (at - s1)];
        } else if (at == end) {
            byte = 0x80;
        }
        v |= byte << (le ? 8 * b : 24 - 8 * b);
    }
    // the bit length, key block included: below 2^32, the words above it stay 0
    if (wi == (le ? words - 2 : words - 1)) v = (block + end) * 8u;
    return v;
}

// Packs the templates of n sessions into scratch taken from sc: ``words`` words
// a session, laid out by ``kernel`` (the file's own pack kernel) under geometry g.
template <class G>
int pack_templates(void (*kernel)(Pack, G), const G& g, const uint8_t* label, size_t labellen, const uint8_t* seed0,
                   size_t len0, const uint8_t* seed1, size_t len1, uint64_t n, Scratch& sc, Pack* p, hipStream_t s) {
    *p = Pack{};
    for (size_t k = 0; k < labellen; ++k) p->label[k >> 2] |= (uint32_t)label[k] << (8 * (k & 3));
    p->labellen = (uint32_t)labellen;
    p->seed0 = seed0;
    p->len0 = (uint32_t)len0;
    p->seed1 = seed1;
    p->len1 = (uint32_t)len1;
    p->n = n;
    p->words = g.words();
    const size_t bytes = (size_t)p->words * 4 * n;
    if (int rc = sc.alloc(bytes)) return rc;
    p->tmpl = sc.take<uint32_t>(bytes, 256);
    const uint64_t threads = (uint64_t)p->words * n;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, *p, g);
    return launched() ? TG_OK : TG_EHIP;
}

// One derivation over templates: scratch, the pack launch, ``launch(tmpl)`` (0
// or a TG_ code) and the scratch's release behind it.  packmsg / launchmsg: the
// error text when the first / the second fails.
template <class G, class F>
int with_templates(void (*kernel)(Pack, G), const G& g, const uint8_t* label, size_t labellen, const uint8_t* seed0,
                   size_t len0, const uint8_t* seed1, size_t len1, uint64_t n, hipStream_t s, const char* packmsg,
                   const char* launchmsg, F launch) {
    Scratch sc(s);
    Pack p;
    int rc = pack_templates(kernel, g, label, labellen, seed0, len0, seed1, len1, n, sc, &p, s);
    if (rc) return fail(rc, "%s", packmsg);
    rc = launch(p.tmpl);
    if (rc) return fail(rc, "%s", launchmsg);
    rc = sc.release();
    return rc ? fail(rc, "scratch release failed") : TG_OK;
}

// The argument errors tg_tls12_prf and tg_tls10_prf share, in their order.
inline int prf_args_error(size_t secretlen, size_t maxsecret, size_t labellen, const uint8_t* label, size_t seedlen,
                          size_t outlen, uint64_t n) {
    if (secretlen == 0 || secretlen > maxsecret)
        return fail(TG_EINVAL, "secret length must be 1..%zu, got %zu", maxsecret, secretlen);
    if (labellen > 32) return fail(TG_EINVAL, "label length must be at most 32, got %zu", labellen);
    if (seedlen > 128) return fail(TG_EINVAL, "seed length must be at most 128, got %zu", seedlen);
    if (outlen == 0 || outlen > 256) return fail(TG_EINVAL, "output length must be 1..256, got %zu", outlen);
    if (labellen && !label) return fail(TG_EINVAL, "null label");
    if (n > kMaxSessions) return fail(TG_EINVAL, "n must be at most 2^31");
    return TG_OK;
}

// ---- the checks of a tg_tls12_install -------------------------------------------
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
