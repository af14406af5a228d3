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
// This is the design of tls12.hip with one addition (the shared text is
// prf_dev.h's and keysetup_dev.h's, as there).  tls10_pack_kernel lays
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

__global__ __launch_bounds__(256) void tls10_pack_kernel(Pack p, Tls10Geom g) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= p.n * p.words) return;
    const uint64_t i = gid % p.n;
    const uint32_t w = (uint32_t)(gid / p.n);
    // which of the four templates, and the word's place in it
    const uint32_t e0 = 16 * g.nb1, e1 = e0 + 16 * g.nbm2, e2 = e1 + 16 * g.nb1;
    const bool le = w < e1;                         // the MD5 pair comes first
    const bool second = le ? w >= e0 : w >= e2;     // A(i) || A(0)
    const uint32_t base = w < e0 ? 0u : w < e1 ? e0 : w < e2 ? e1 : e2;
    const uint32_t words = w < e0 ? e0 : w < e1 ? e1 - e0 : w < e2 ? e2 - e1 : p.words - e2;
    const uint32_t hole = second ? (le ? (uint32_t)Md5::kHash : (uint32_t)Sha1::kHash) : 0u;
    p.tmpl[(uint64_t)w * p.n + i] = pack_word(p, i, w - base, hole, words, 64u, le);
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
    const uint8_t* sec = secrets + (uint64_t)secretlen * i;
    const uint32_t half = (secretlen + 1) / 2, at2 = secretlen - half;   // S1 = [0, half), S2 = [at2, L)
    Hm<Md5> hm;
    Hm<Sha1> hs;
    {
        uint32_t key[16];
        key_from_bytes<Md5>(sec, half, key);
        hm_key<Md5>(key, hm);
        key_from_bytes<Sha1>(sec + at2, half, key);
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
        uint32_t key[16];   // S1: the master secret's first 24 bytes
        key_from_row<Md5, 24>(ms + 48 * j, key);
        Hm<Md5> h;
        hm_key<Md5>(key, h);
        p_hash_words<Md5, NBM>(h, t.m1, g.nb1, t.m2, g.nbm2, n, kb);
    }
    {
        uint32_t key[16];   // S2: its last 24 bytes
        key_from_row<Sha1, 24>(ms + 48 * j + 24, key);
        Hm<Sha1> h;
        hm_key<Sha1>(key, h);
        uint32_t ks[NBS * 5];
        p_hash_words<Sha1, NBS>(h, t.s1, g.nb1, t.s2, g.nbs2, n, ks);
#pragma unroll
        for (int k = 0; k < NEED; ++k) kb[k] ^= ks[k];
    }
    const bool server = side != 0;
    uint32_t mk[MW], m[16], rk[60];
    side_words<MW>(kb, 0, server, mk);
    mac_words<Sha1>(mk, m);
    side_words<NK>(kb, 2 * MW, server, rk);
#pragma unroll
    for (int k = 0; k < NK; ++k) rk[k] = bswap32(rk[k]);
    if (seq_next) seq_next[s] = 0;
    store_cbc_row<NK, Sha1>(sb, rk, m, rows + s, (uint32_t)TG_MAC_SHA1);
}

}  // namespace
}  // namespace tg

using tg::fail;

extern "C" {

int tg_tls10_prf(const uint8_t* secrets, size_t secretlen, uint64_t n, const uint8_t* label, size_t labellen,
                 const uint8_t* seeds, size_t seedlen, size_t outlen, uint8_t* out, void* stream) {
    if (int rc = tg::prf_args_error(secretlen, 128, labellen, label, seedlen, outlen, n)) return rc;
    if (n == 0) return TG_OK;
    if (!secrets || !out || (seedlen && !seeds)) return fail(TG_EINVAL, "null device buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const tg::Tls10Geom g = tg::tls10_geom(labellen + seedlen);
    return tg::with_templates(tg::tls10_pack_kernel, g, label, labellen, seeds, seedlen, nullptr, 0, n, s,
                              "PRF template launch failed", "PRF launch failed", [&](const uint32_t* tmpl) {
                                  hipLaunchKernelGGL(tg::tls10_prf_kernel, dim3(tg::blocks_of(n)), dim3(256), 0, s,
                                                     tmpl, g, secrets, (uint32_t)secretlen, n, (uint32_t)outlen, out);
                                  return tg::launched() ? TG_OK : TG_EHIP;
                              });
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
    const tg::Tls10Geom g = tg::tls10_geom(13 + 32 + 32);
    const char* msg = "TLS 1.1 CBC install launch failed";
    return tg::with_templates(
        tg::tls10_pack_kernel, g, tg::kKeyExpansion, 13, r->server_random, 32, r->client_random, 32, r->n, s, msg, msg,
        [&](const uint32_t* tmpl) {
            if (k->rounds == 10)
                hipLaunchKernelGGL(tg::tls11_cbcrow_install_kernel<4>, dim3(tg::blocks_of(r->n)), dim3(256), 0, s, tmpl,
                                   g, r->slot, r->master_secrets, r->side, r->seq_next, r->n, (uint64_t)k->nkeys,
                                   k->dev_key);
            else
                hipLaunchKernelGGL(tg::tls11_cbcrow_install_kernel<8>, dim3(tg::blocks_of(r->n)), dim3(256), 0, s, tmpl,
                                   g, r->slot, r->master_secrets, r->side, r->seq_next, r->n, (uint64_t)k->nkeys,
                                   k->dev_key);
            return tg::launched() ? TG_OK : TG_EHIP;
        });
}

}  // extern "C"
