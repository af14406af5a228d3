// tls10.hip -- TLS 1.0 / 1.1 key setup on the device: the MD5 xor SHA-1 PRF
// and the install of its key block into live CBC table rows, so a TLS 1.1
// session's keys never visit the host (tg_tls10_prf,
// tg_cbc_sessions_install_tls11).
//
// Restates, one session per lane:
//   PRF (tlslite/mathtls.py:701-714): S1 = the first ceil(L / 2) bytes of the
//     secret, S2 = the last ceil(L / 2) (they share the middle byte of an odd
//     L), out = P_hash(md5, S1, label || seed) xor P_hash(sha1, S2, label ||
//     seed), byte by byte; P_hash as tls12.hip restates it (:679-698).
//   RecordLayer.calcPendingStates (recordlayer.py:1189-1246) at version (3, 2):
//     the key block PRF(master secret, "key expansion", server_random ||
//     client_random) cut as client MAC, server MAC, client key, server key.
//
// This is the design of tls12.hip with one addition.  tls10_pack_kernel lays
// the public messages out once in library scratch, word w of session i at
// tmpl[w * n + i]: A(0) and A(i) || A(0), each padded once for MD5
// (little-endian words, the length in word 14, a 16-byte hole for A(i)) and
// once for SHA-1 (big-endian, the length in word 15, a 20-byte hole) -- four
// templates, in that order.  They hold label and seed only.  Each half of the
// secret enters as two HMAC midstates; A(i), both output streams and their
// xor stay in registers.
//
// The two P_hash streams advance at different strides, 16 and 20 bytes per
// iteration: outlen bytes take ceil(outlen / 16) MD5 iterations and
// ceil(outlen / 20) SHA-1 iterations.  tls10_prf_kernel works in chunks of 80
// bytes, where both streams end together: up to five MD5 digests and up to
// four SHA-1 digests shift into two 20-word windows (compile-time indices
// inside loops that are not unrolled; an iteration past outlen is skipped, a
// uniform branch on the lengths), the windows are xored word by word and the
// chunk's bytes are stored.  One lane runs both chains, one after the other:
// both are dependent chains of 32-bit adds, rotates and logic ops with no
// long-latency instruction in them, and the SIMD issues one wave's next VALU
// instruction as soon as the previous one's result is there, so a second
// chain interleaved into the same lane would have nothing to hide; a split
// over two lanes would cost a cross-lane exchange per output word and halve
// the sessions per wave.  DESIGN.md section 3.18 has the measurement.
//
// Every loop's trip count depends on lengths alone, and nothing is held in an
// array indexed at run time: no kernel here has a private segment.
#include "md5.h"
#include "prf_dev.h"

namespace tg {
namespace {

// ---- the four message templates ---------------------------------------------
// Both hashes have 64-byte blocks and an 8-byte length: A(0) takes nb1 blocks
// for either; A(i) || A(0) takes nbm2 (MD5) or nbs2 (SHA-1).
struct Tls10Geom {
    uint32_t nb1, nbm2, nbs2;
    __host__ __device__ uint32_t words() const { return (2 * nb1 + nbm2 + nbs2) * 16; }
};

Tls10Geom tls10_geom(size_t msglen) {
    Tls10Geom g;
    g.nb1 = (uint32_t)((msglen + 8) / 64 + 1);
    g.nbm2 = (uint32_t)((Md5::kHash + msglen + 8) / 64 + 1);
    g.nbs2 = (uint32_t)((Sha1::kHash + msglen + 8) / 64 + 1);
    return g;
}

struct Tls10Pack {
    uint32_t label[8];      // LE words of the label's bytes
    uint32_t labellen;
    uint32_t len0, len1;    // the seed is row i of seed0 then row i of seed1
    const uint8_t* seed0;
    const uint8_t* seed1;
    Tls10Geom g;
    uint64_t n;
    uint32_t* tmpl;
};

__global__ __launch_bounds__(256) void tls10_pack_kernel(Tls10Pack p) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t wt = p.g.words();
    if (gid >= p.n * wt) return;
    const uint64_t i = gid % p.n;
    const uint32_t w = (uint32_t)(gid / p.n);
    // which of the four templates, and the word's place in it
    const uint32_t e0 = 16 * p.g.nb1, e1 = e0 + 16 * p.g.nbm2, e2 = e1 + 16 * p.g.nb1;
    const bool le = w < e1;                         // the MD5 pair comes first
    const bool second = le ? w >= e0 : w >= e2;     // A(i) || A(0)
    const uint32_t base = w < e0 ? 0u : w < e1 ? e0 : w < e2 ? e1 : e2;
    const uint32_t words = w < e0 ? e0 : w < e1 ? e1 - e0 : w < e2 ? e2 - e1 : wt - e2;
    const uint32_t wi = w - base;
    const uint32_t hole = second ? (le ? (uint32_t)Md5::kHash : (uint32_t)Sha1::kHash) : 0u;
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
    // the bit length, key block included: below 2^32, its high word stays 0
    if (wi == (le ? words - 2 : words - 1)) v = (64u + end) * 8u;
    p.tmpl[(uint64_t)w * p.n + i] = v;
}

// This lane's word 0 of each template.
struct Tls10Tmpl {
    const uint32_t *m1, *m2, *s1, *s2;
};

__device__ __forceinline__ Tls10Tmpl tls10_tmpl(const uint32_t* tmpl, Tls10Geom g, uint64_t n, uint64_t i) {
    Tls10Tmpl t;
    t.m1 = tmpl + i;
    t.m2 = t.m1 + (uint64_t)16 * g.nb1 * n;
    t.s1 = t.m2 + (uint64_t)16 * g.nbm2 * n;
    t.s2 = t.s1 + (uint64_t)16 * g.nb1 * n;
    return t;
}

// ---- tg_tls10_prf ------------------------------------------------------------
__global__ __launch_bounds__(256) void tls10_prf_kernel(const uint32_t* __restrict__ tmpl, Tls10Geom g,
                                                        const uint8_t* __restrict__ secrets, uint32_t secretlen,
                                                        uint64_t n, uint32_t outlen, uint8_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const gptr_c sec = (gptr_c)(secrets + (uint64_t)secretlen * i);
    const uint32_t half = (secretlen + 1) / 2, at2 = secretlen - half;   // S1 = [0, half), S2 = [at2, L)
    Hm<Md5> hm;
    Hm<Sha1> hs;
    {
        uint32_t key[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t at = (uint32_t)(4 * k + b);
                uint32_t byte = 0;
                if (at < half) byte = sec[at];
                v |= byte << (8 * b);
            }
            key[k] = v;
        }
        hm_key<Md5>(key, hm);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t at = (uint32_t)(4 * k + b);
                uint32_t byte = 0;
                if (at < half) byte = sec[at2 + at];
                v = (v << 8) | byte;
            }
            key[k] = v;
        }
        hm_key<Sha1>(key, hs);
    }
    const Tls10Tmpl t = tls10_tmpl(tmpl, g, n, i);
    uint32_t am[8], as[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = 0;
    hm_tmpl<Md5, false>(hm, t.m1, n, g.nb1, o, am);            // A(1) of either chain
    hm_tmpl<Sha1, false>(hs, t.s1, n, g.nb1, o, as);
    const gptr op = (gptr)(out + (uint64_t)outlen * i);
#pragma unroll 1
    for (uint32_t pos = 0; pos < outlen; pos += 80) {           // uniform
        uint32_t x[20], y[20];   // the chunk's bytes of either stream as LE words
#pragma unroll
        for (int k = 0; k < 20; ++k) x[k] = y[k] = 0;
#pragma unroll 1
        for (uint32_t q = 0; q < 5; ++q) {
            const uint32_t at = pos + 16 * q;
            uint32_t d[4] = {0, 0, 0, 0};
            if (at < outlen) {                                  // uniform
                hm_tmpl<Md5, true>(hm, t.m2, n, g.nbm2, am, o);
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = o[k];
                if (at + 16 < outlen) {
                    hm_digest<Md5>(hm, am, o);
#pragma unroll
                    for (int k = 0; k < 8; ++k) am[k] = o[k];
                }
            }
            // the window moves down one digest; after five rounds digest 0 is at x[0]
#pragma unroll
            for (int k = 0; k < 16; ++k) x[k] = x[k + 4];
#pragma unroll
            for (int k = 0; k < 4; ++k) x[16 + k] = d[k];
        }
#pragma unroll 1
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t at = pos + 20 * q;
            uint32_t d[5] = {0, 0, 0, 0, 0};
            if (at < outlen) {                                  // uniform
                hm_tmpl<Sha1, true>(hs, t.s2, n, g.nbs2, as, o);
#pragma unroll
                for (int k = 0; k < 5; ++k) d[k] = bswap32(o[k]);
                if (at + 20 < outlen) {
                    hm_digest<Sha1>(hs, as, o);
#pragma unroll
                    for (int k = 0; k < 8; ++k) as[k] = o[k];
                }
            }
#pragma unroll
            for (int k = 0; k < 15; ++k) y[k] = y[k + 5];
#pragma unroll
            for (int k = 0; k < 5; ++k) y[15 + k] = d[k];
        }
#pragma unroll
        for (int k = 0; k < 80; ++k)
            if (pos + k < outlen) op[pos + k] = (uint8_t)((x[k / 4] ^ y[k / 4]) >> (8 * (k % 4)));
    }
}

// ---- tg_cbc_sessions_install_tls11 -------------------------------------------
// Lane j rebuilds row slot[j] of an HMAC-SHA1 table from the key block of master
// secret j: 2 * 20 + 2 * 4 * NK bytes, 5 / 7 MD5 digests and 4 / 6 SHA-1 digests
// for NK = 4 / 8.  The 16-byte IV blocks behind the keys are not derived:
// unused at TLS >= 1.1.
template <int NK>
__global__ __launch_bounds__(256) void tls11_cbcrow_install_kernel(const uint32_t* __restrict__ tmpl, Tls10Geom g,
                                                                const uint32_t* __restrict__ slot,
                                                                const uint8_t* __restrict__ ms, uint32_t side,
                                                                uint64_t* __restrict__ seq_next, uint64_t n,
                                                                uint64_t nkeys, CbcKeyDev* rows) {
    constexpr int MW = Sha1::kHash / 4, NEED = 2 * MW + 2 * NK;
    constexpr int NBM = (NEED + 3) / 4, NBS = (NEED + 4) / 5;
    __shared__ uint8_t sb[256];
    for (int k = threadIdx.x; k < 256; k += blockDim.x) sb[k] = c_sbox.s[k];
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t s = slot ? (uint64_t)slot[j] : j;
    if (s >= nkeys) return;
    const Tls10Tmpl t = tls10_tmpl(tmpl, g, n, j);
    uint32_t kb[NBM * 4];   // big-endian words of the key block's bytes
    {
        uint32_t key[16];   // S1: the master secret's first 24 bytes, LE words
#pragma unroll
        for (int k = 0; k < 16; ++k) key[k] = k < 6 ? load_u32u(ms + 48 * j + 4 * k) : 0u;
        Hm<Md5> h;
        hm_key<Md5>(key, h);
        p_hash_words<Md5, NBM>(h, t.m1, g.nb1, t.m2, g.nbm2, n, kb);
    }
    {
        uint32_t key[16];   // S2: its last 24 bytes, big-endian words
#pragma unroll
        for (int k = 0; k < 16; ++k) key[k] = k < 6 ? bswap32(load_u32u(ms + 48 * j + 24 + 4 * k)) : 0u;
        Hm<Sha1> h;
        hm_key<Sha1>(key, h);
        uint32_t ks[NBS * 5];
        p_hash_words<Sha1, NBS>(h, t.s1, g.nb1, t.s2, g.nbs2, n, ks);
#pragma unroll
        for (int k = 0; k < NEED; ++k) kb[k] ^= ks[k];
    }
    const bool server = side != 0;
    uint32_t m[16];   // the MAC key, big-endian words, zero-padded
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < MW) {   // both sides' words as values, then the select
            const uint32_t c = kb[k], sv = kb[MW + k];
            m[k] = server ? sv : c;
        } else {
            m[k] = 0u;
        }
    }
    uint32_t rk[60];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const uint32_t c = kb[2 * MW + k], sv = kb[2 * MW + NK + k];
        rk[k] = bswap32(server ? sv : c);
    }
    if (seq_next) seq_next[s] = 0;
    store_cbc_row<NK, Sha1>(sb, rk, m, rows + s, (uint32_t)TG_MAC_SHA1);
}

// ---- launchers -------------------------------------------------------------------
// Packs the four templates of n sessions into scratch taken from sc.
int pack_templates(const uint8_t* label, size_t labellen, const uint8_t* seed0, size_t len0, const uint8_t* seed1,
                   size_t len1, uint64_t n, Scratch& sc, Tls10Pack* p, hipStream_t s) {
    *p = Tls10Pack{};
    for (size_t k = 0; k < labellen; ++k) p->label[k >> 2] |= (uint32_t)label[k] << (8 * (k & 3));
    p->labellen = (uint32_t)labellen;
    p->seed0 = seed0;
    p->len0 = (uint32_t)len0;
    p->seed1 = seed1;
    p->len1 = (uint32_t)len1;
    p->g = tls10_geom(labellen + len0 + len1);
    p->n = n;
    const size_t bytes = (size_t)p->g.words() * 4 * n;
    if (int rc = sc.alloc(bytes)) return rc;
    p->tmpl = sc.take<uint32_t>(bytes, 256);
    const uint64_t threads = (uint64_t)p->g.words() * n;
    hipLaunchKernelGGL(tls10_pack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, *p);
    return launched() ? TG_OK : TG_EHIP;
}

}  // namespace
}  // namespace tg

using tg::fail;

extern "C" {

int tg_tls10_prf(const uint8_t* secrets, size_t secretlen, uint64_t n, const uint8_t* label, size_t labellen,
                 const uint8_t* seeds, size_t seedlen, size_t outlen, uint8_t* out, void* stream) {
    if (secretlen == 0 || secretlen > 128)
        return fail(TG_EINVAL, "secret length must be 1..128, got %zu", secretlen);
    if (labellen > 32) return fail(TG_EINVAL, "label length must be at most 32, got %zu", labellen);
    if (seedlen > 128) return fail(TG_EINVAL, "seed length must be at most 128, got %zu", seedlen);
    if (outlen == 0 || outlen > 256) return fail(TG_EINVAL, "output length must be 1..256, got %zu", outlen);
    if (labellen && !label) return fail(TG_EINVAL, "null label");
    if (n > tg::kMaxSessions) return fail(TG_EINVAL, "n must be at most 2^31");
    if (n == 0) return TG_OK;
    if (!secrets || !out || (seedlen && !seeds)) return fail(TG_EINVAL, "null device buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    tg::Scratch sc(s);
    tg::Tls10Pack p;
    int rc = tg::pack_templates(label, labellen, seeds, seedlen, nullptr, 0, n, sc, &p, s);
    if (rc) return fail(rc, "PRF template launch failed");
    hipLaunchKernelGGL(tg::tls10_prf_kernel, dim3(tg::blocks_of(n)), dim3(256), 0, s, p.tmpl, p.g, secrets,
                       (uint32_t)secretlen, n, (uint32_t)outlen, out);
    if (!tg::launched()) return fail(TG_EHIP, "PRF launch failed");
    rc = sc.release();
    return rc ? fail(rc, "scratch release failed") : TG_OK;
}

int tg_cbc_sessions_install_tls11(tg_cbc_key* k, const tg_tls12_install* r, void* stream) {
    if (int rc = tg::install_struct_error(r, false, false)) return rc;
    if (!k) return fail(TG_EINVAL, "null key");
    if (int rc = tg::install_count_error(r, k->nkeys)) return rc;
    if (k->mac != TG_MAC_SHA1)
        return fail(TG_EINVAL, "no TLS 1.1 suite the engine runs has this handle's MAC (HMAC-%s): HMAC-SHA1 only",
                    k->mac == TG_MAC_SHA256 ? "SHA256" : "SHA384");
    if (r->n == 0) return TG_OK;
    if (int rc = tg::cbc_select_device(k)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    tg::Scratch sc(s);
    tg::Tls10Pack p;
    int rc = tg::pack_templates(tg::kKeyExpansion, 13, r->server_random, 32, r->client_random, 32, r->n, sc, &p, s);
    if (!rc) {
        if (k->rounds == 10)
            hipLaunchKernelGGL(tg::tls11_cbcrow_install_kernel<4>, dim3(tg::blocks_of(r->n)), dim3(256), 0, s, p.tmpl,
                               p.g, r->slot, r->master_secrets, r->side, r->seq_next, r->n, (uint64_t)k->nkeys,
                               k->dev_key);
        else
            hipLaunchKernelGGL(tg::tls11_cbcrow_install_kernel<8>, dim3(tg::blocks_of(r->n)), dim3(256), 0, s, p.tmpl,
                               p.g, r->slot, r->master_secrets, r->side, r->seq_next, r->n, (uint64_t)k->nkeys,
                               k->dev_key);
        if (!tg::launched()) rc = TG_EHIP;
    }
    if (rc) return fail(rc, "TLS 1.1 CBC install launch failed");
    rc = sc.release();
    return rc ? fail(rc, "scratch release failed") : TG_OK;
}

}  // extern "C"
