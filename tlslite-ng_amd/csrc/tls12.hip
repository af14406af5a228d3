// tls12.hip -- TLS 1.2 key setup on the device: the PRF, the key block and
// the installs of its slices into live key tables, so a TLS 1.2 session's
// keys never visit the host (tg_tls12_prf, tg_cbc_key_create_device,
// tg_cbc_key_replace_device, tg_sessions_install_tls12,
// tg_cbc_sessions_install_tls12).
//
// Restates, one session per lane:
//   P_hash (tlslite/mathtls.py:679-698) as PRF_1_2 / PRF_1_2_SHA384 (:716-722)
//     call it: A(0) = label || seed, A(i) = HMAC(secret, A(i-1)),
//     out = HMAC(secret, A(1) || A(0)) || HMAC(secret, A(2) || A(0)) || ...
//   RecordLayer.calcPendingStates (recordlayer.py:1189-1246): the key block
//     P_hash(master secret, "key expansion" || server_random || client_random)
//     cut as client MAC, server MAC, client key, server key, client IV,
//     server IV, with the lengths of _getCipherSettings / _getMacSettings.
//
// Layout.  Two messages are hashed again and again per session: A(0), and
// A(i) || A(0).  prf_pack_kernel lays both out once, SHA-padded and with their
// length fields, as big-endian words in library scratch -- word w of session
// i at tmpl[w * n + i], so a wave reads a word of 64 sessions in one line.
// The second template starts with a hole of one digest: A(i) is a whole number
// of words and is spliced in from registers with compile-time indices.  The
// templates hold label and seed only (public handshake values); the secret
// enters as the two HMAC midstates, computed once per lane, and A(i), the
// outputs and the raw keys of the fused installs stay in registers.  Every
// loop's trip count depends on lengths alone, and nothing is held in an array
// indexed at run time: no kernel here has a private segment.
//
// The fused installs collect the key block's words in a register window that
// shifts down by one digest per output block (compile-time indices inside a
// loop that is not unrolled), pick their side's slices with selects, then run
// the AES key schedule and the entry store of keysetup_dev.h, or build a
// CbcKeyDev row: forward schedule, the equivalent inverse cipher's schedule
// (build_row of aes_cbc.hip) and the two HMAC midstates of the MAC key.
//
// Nothing of that is this file's own text: the HMAC core and the key loads are
// keysetup_dev.h's, the template HMAC, P_hash into the window (p_hash_words),
// the slice selects, the row store and the packer's word are prf_dev.h's,
// which tls10.hip (the TLS 1.0 / 1.1 PRF) shares.  Here are the geometry of the
// two templates, the kernels and their launches.
#include "keys.h"
#include "prf_dev.h"

#include <new>

namespace tg {
namespace {

// ---- the two message templates ---------------------------------------------
struct PrfGeom {
    uint32_t hashlen, block, nb1, nb2;
    __host__ __device__ uint32_t words() const { return (nb1 + nb2) * (block / 4); }
};

PrfGeom prf_geom(int hashlen, size_t msglen) {
    PrfGeom g;
    g.hashlen = (uint32_t)hashlen;
    g.block = hashlen == 32 ? 64 : 128;
    const uint32_t lenbytes = g.block / 8;
    g.nb1 = (uint32_t)((msglen + lenbytes) / g.block + 1);
    g.nb2 = (uint32_t)((hashlen + msglen + lenbytes) / g.block + 1);
    return g;
}

// Word w of a session: the template of A(0), then that of A(i) || A(0).
__global__ __launch_bounds__(256) void prf_pack_kernel(Pack p, PrfGeom g) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= p.n * p.words) return;
    const uint64_t i = gid % p.n;
    const uint32_t w = (uint32_t)(gid / p.n), w1 = g.nb1 * (g.block / 4);
    const bool second = w >= w1;
    p.tmpl[(uint64_t)w * p.n + i] = pack_word(p, i, second ? w - w1 : w, second ? g.hashlen : 0u,
                                              second ? p.words - w1 : w1, g.block, false);
}

// ---- tg_tls12_prf ------------------------------------------------------------
template <class H>
__global__ __launch_bounds__(256) void tls12_prf_kernel(const uint32_t* __restrict__ tmpl, uint32_t nb1, uint32_t nb2,
                                                        const uint8_t* __restrict__ secrets, uint32_t secretlen,
                                                        uint64_t n, uint32_t outlen, uint8_t* __restrict__ out) {
    using W = typename H::word;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Hm<H> h;
    {
        W key[16];
        key_from_bytes<H>(secrets + (uint64_t)secretlen * i, secretlen, key);
        hm_key<H>(key, h);
    }
    const uint32_t* t1 = tmpl + i;
    const uint32_t* t2 = tmpl + (uint64_t)nb1 * (H::kBlock / 4) * n + i;
    W a[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = 0;
    hm_tmpl<H, false>(h, t1, n, nb1, a, o);                 // A(1)
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = o[k];
    uint8_t* op = out + (uint64_t)outlen * i;
    for (uint32_t pos = 0; pos < outlen; pos += H::kHash) { // uniform
        hm_tmpl<H, true>(h, t2, n, nb2, a, o);
        store_digest_bytes<H>(o, op + pos, outlen - pos);
        if (pos + H::kHash < outlen) {
            hm_digest<H>(h, a, o);
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] = o[k];
        }
    }
}

// ---- the key block in registers ----------------------------------------------
// The first NB digests of P_hash(master secret j, template) as big-endian
// 32-bit words of the key block's bytes.
template <class H, int NB>
__device__ __forceinline__ void key_block(const uint32_t* __restrict__ tmpl, uint32_t nb1, uint32_t nb2,
                                          const uint8_t* __restrict__ ms, uint64_t n, uint64_t j,
                                          uint32_t kb[NB * (H::kHash / 4)]) {
    typename H::word key[16];
    key_from_row<H, 48>(ms + 48 * j, key);
    Hm<H> h;
    hm_key<H>(key, h);
    p_hash_words<H, NB>(h, tmpl + j, nb1, tmpl + (uint64_t)nb1 * (H::kBlock / 4) * n + j, nb2, n, kb);
}

// ---- tg_sessions_install_tls12 -----------------------------------------------
// Lane j installs the AEAD key and fixed IV of its side into entry slot[j].
// NK / LAYOUT as rekey_kernel's (keysetup.hip); ivw: IV words, 1 or 3.
template <class H, int NK, int LAYOUT>
__global__ __launch_bounds__(256) void tls12_install_kernel(const uint32_t* __restrict__ tmpl, uint32_t nb1,
                                                            uint32_t nb2, const uint32_t* __restrict__ slot,
                                                            const uint8_t* __restrict__ ms, uint32_t side,
                                                            uint32_t ivw, uint8_t* __restrict__ iv_table,
                                                            uint64_t* __restrict__ seq_next, uint64_t n,
                                                            uint64_t nkeys, void* out) {
    constexpr int KW = NK ? NK : 8, HW = H::kHash / 4;
    constexpr int NEED = 2 * KW + 6, NB = (NEED + HW - 1) / HW;   // both keys, both 12-byte IVs
    __shared__ uint8_t sb[256];
    if (NK) {
        for (int k = threadIdx.x; k < 256; k += blockDim.x) sb[k] = c_sbox.s[k];
        __syncthreads();
    }
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t s = slot ? (uint64_t)slot[j] : j;
    if (s >= nkeys) return;
    uint32_t kb[NB * HW];
    key_block<H, NB>(tmpl, nb1, nb2, ms, n, j, kb);
    const bool server = side != 0, iv12 = ivw == 3;
    uint32_t rk[60];   // rk[0 .. KW): the key as LE words of its bytes
    side_words<KW>(kb, 0, server, rk);
#pragma unroll
    for (int k = 0; k < KW; ++k) rk[k] = bswap32(rk[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // the IV as side_words picks: values first, then the selects
        const uint32_t c = kb[2 * KW + k], s4 = kb[2 * KW + 1 + k], s12 = kb[2 * KW + 3 + k];
        const uint32_t sv = iv12 ? s12 : s4;
        const uint32_t v = server ? sv : c;
        if ((uint32_t)k < ivw) store_u32u(iv_table + 4 * (uint64_t)ivw * s + 4 * k, bswap32(v));
    }
    if (seq_next) seq_next[s] = 0;
    if constexpr (NK == 0) {
        ChachaKeyDev* o = static_cast<ChachaKeyDev*>(out) + s;
#pragma unroll
        for (int k = 0; k < 8; ++k) o->k[k] = rk[k];
    } else {
        expand_words<NK>(sb, rk);
        store_aes_entry<NK, LAYOUT>(sb, rk, out, s);
    }
}

// ---- CBC rows (store_cbc_row: prf_dev.h) ----------------------------------------
// tg_cbc_key_create_device / tg_cbc_key_replace_device: row slot[j] from the
// raw keys of row j.  (Named cbcrows / cbcrow, not cbc_...: the metadata test
// of aes_cbc.hip counts that file's kernels by the pattern cbc_*_kernel.)
template <int NK, class HM>
__global__ __launch_bounds__(256) void cbcrows_kernel(const uint32_t* __restrict__ slot,
                                                       const uint8_t* __restrict__ enc_keys,
                                                       const uint8_t* __restrict__ mac_keys, uint32_t mackeylen,
                                                       uint64_t n, uint64_t nkeys, CbcKeyDev* rows, uint32_t mac) {
    __shared__ uint8_t sb[256];
    for (int k = threadIdx.x; k < 256; k += blockDim.x) sb[k] = c_sbox.s[k];
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t s = slot ? (uint64_t)slot[j] : j;
    if (s >= nkeys) return;
    uint32_t rk[60];
#pragma unroll
    for (int k = 0; k < NK; ++k) rk[k] = load_u32u(enc_keys + 4 * NK * j + 4 * k);
    typename HM::word m[16];
    key_from_bytes<HM>(mac_keys + (uint64_t)mackeylen * j, mackeylen, m);
    store_cbc_row<NK, HM>(sb, rk, m, rows + s, mac);
}

// ---- tg_cbc_sessions_install_tls12 -------------------------------------------
// HP: the suite's PRF hash; HM: the table's MAC (its digest length is the MAC
// key's length).  The 16-byte IV blocks behind the keys are not derived: unused
// at TLS >= 1.1.
template <class HP, int NK, class HM>
__global__ __launch_bounds__(256) void tls12_cbcrow_install_kernel(const uint32_t* __restrict__ tmpl, uint32_t nb1,
                                                                uint32_t nb2, const uint32_t* __restrict__ slot,
                                                                const uint8_t* __restrict__ ms, uint32_t side,
                                                                uint64_t* __restrict__ seq_next, uint64_t n,
                                                                uint64_t nkeys, CbcKeyDev* rows, uint32_t mac) {
    constexpr int HW = HP::kHash / 4, MW = HM::kHash / 4;
    constexpr int NEED = 2 * MW + 2 * NK, NB = (NEED + HW - 1) / HW;
    __shared__ uint8_t sb[256];
    for (int k = threadIdx.x; k < 256; k += blockDim.x) sb[k] = c_sbox.s[k];
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t s = slot ? (uint64_t)slot[j] : j;
    if (s >= nkeys) return;
    uint32_t kb[NB * HW];
    key_block<HP, NB>(tmpl, nb1, nb2, ms, n, j, kb);
    const bool server = side != 0;
    uint32_t mk[MW], rk[60];
    typename HM::word m[16];
    side_words<MW>(kb, 0, server, mk);
    mac_words<HM>(mk, m);
    side_words<NK>(kb, 2 * MW, server, rk);
#pragma unroll
    for (int k = 0; k < NK; ++k) rk[k] = bswap32(rk[k]);
    if (seq_next) seq_next[s] = 0;
    store_cbc_row<NK, HM>(sb, rk, m, rows + s, mac);
}

// ---- launchers -------------------------------------------------------------------
template <class H>
int launch_install(tg_key* k, const uint32_t* tmpl, const PrfGeom& g, const tg_tls12_install& r, hipStream_t s) {
    const int layout = k->alg == TG_CHACHA20_POLY1305 ? 3 : is_ccm(k->alg) ? 2 : (k->nkeys > 1 ? 1 : 0);
#define TG_INSTALL(NK, L)                                                                                   \
    hipLaunchKernelGGL((tls12_install_kernel<H, NK, L>), dim3(blocks_of(r.n)), dim3(256), 0, s, tmpl,       \
                       g.nb1, g.nb2, r.slot, r.master_secrets, r.side, r.fixed_iv_len / 4, r.iv_table,      \
                       r.seq_next, r.n, (uint64_t)k->nkeys, k->dev_key)
    if constexpr (H::kHash == 48) {   // aead_pair_ok: AES-256-GCM only
        if (layout == 0) TG_INSTALL(8, 0);
        else TG_INSTALL(8, 1);
    } else if (layout == 3) {
        TG_INSTALL(0, 3);
    } else if (k->keylen == 16) {
        if (layout == 0) TG_INSTALL(4, 0);
        else if (layout == 1) TG_INSTALL(4, 1);
        else TG_INSTALL(4, 2);
    } else {
        if (layout == 0) TG_INSTALL(8, 0);
        else if (layout == 1) TG_INSTALL(8, 1);
        else TG_INSTALL(8, 2);
    }
#undef TG_INSTALL
    if (!launched()) return TG_EHIP;
    if (layout == 0) return tg_launch_single_rebuild(k->dev_key, r.slot, s);
    if (layout == 1) {   // the table's derived arrays, slot forms
        const auto* keys = static_cast<const GcmTableKey*>(k->dev_key);
        if (int rc = tg_launch_table_hpow(keys, r.n, table_hpow(k), s, r.slot, k->nkeys)) return rc;
        return tg_launch_kt_planes(keys, r.n, k->rounds, table_planes(k), table_rot(k), s, r.slot, k->nkeys);
    }
    return TG_OK;
}

// The (PRF hash, handle) pairs a TLS 1.2 suite can produce (_getCipherSettings,
// _getMacSettings, sha384PrfSuites): the SHA-384 PRF goes with AES-256-GCM and
// with AES-256-CBC + HMAC-SHA384 alone, and HMAC-SHA384 with no other PRF.
// Only these are instantiated; another pair is an argument error.
bool aead_pair_ok(uint32_t hashlen, const tg_key* k) {
    return hashlen == 32 || (k->alg == TG_AES_GCM && k->keylen == 32);
}

bool cbc_pair_ok(uint32_t hashlen, const tg_cbc_key* k) {
    return hashlen == 32 ? k->mac != TG_MAC_SHA384 : (k->mac == TG_MAC_SHA384 && k->rounds == 14);
}

template <class HP, int NK, class HM>
int launch_cbc_install(tg_cbc_key* k, const uint32_t* tmpl, const PrfGeom& g, const tg_tls12_install& r,
                       hipStream_t s) {
#define TG_CBC_INSTALL(HM)                                                                                    \
    hipLaunchKernelGGL((tls12_cbcrow_install_kernel<HP, NK, HM>), dim3(blocks_of(r.n)), dim3(256), 0, s, tmpl,   \
                       g.nb1, g.nb2, r.slot, r.master_secrets, r.side, r.seq_next, r.n,                       \
                       (uint64_t)k->nkeys, k->dev_key, (uint32_t)k->mac)
    TG_CBC_INSTALL(HM);
#undef TG_CBC_INSTALL
    return launched() ? TG_OK : TG_EHIP;
}

template <int NK>
int launch_cbc_rows(int mac, const uint32_t* slot, const uint8_t* enc_keys, const uint8_t* mac_keys,
                    size_t mackeylen, uint64_t n, uint64_t nkeys, CbcKeyDev* rows, hipStream_t s) {
#define TG_CBC_ROWS(HM)                                                                                      \
    hipLaunchKernelGGL((cbcrows_kernel<NK, HM>), dim3(blocks_of(n)), dim3(256), 0, s, slot, enc_keys,       \
                       mac_keys, (uint32_t)mackeylen, n, nkeys, rows, (uint32_t)mac)
    if (mac == TG_MAC_SHA1) TG_CBC_ROWS(Sha1);
    else if (mac == TG_MAC_SHA256) TG_CBC_ROWS(Sha256);
    else TG_CBC_ROWS(Sha384);
#undef TG_CBC_ROWS
    return launched() ? TG_OK : TG_EHIP;
}

int cbc_rows(int rounds, int mac, const uint32_t* slot, const uint8_t* enc_keys, const uint8_t* mac_keys,
             size_t mackeylen, uint64_t n, uint64_t nkeys, CbcKeyDev* rows, hipStream_t s) {
    return rounds == 10 ? launch_cbc_rows<4>(mac, slot, enc_keys, mac_keys, mackeylen, n, nkeys, rows, s)
                        : launch_cbc_rows<8>(mac, slot, enc_keys, mac_keys, mackeylen, n, nkeys, rows, s);
}

// The key block's templates ("key expansion" || server_random || client_random)
// of r's sessions around ``launch(tmpl, g)``; msg: the error text of either launch.
template <class F>
int install_templates(const tg_tls12_install* r, hipStream_t s, const char* msg, F launch) {
    const PrfGeom g = prf_geom((int)r->hashlen, 13 + 32 + 32);
    return with_templates(prf_pack_kernel, g, kKeyExpansion, 13, r->server_random, 32, r->client_random, 32, r->n, s,
                          msg, msg, [&](const uint32_t* tmpl) { return launch(tmpl, g); });
}

}  // namespace
}  // namespace tg

using tg::fail;

extern "C" {

int tg_tls12_prf(int hashlen, const uint8_t* secrets, size_t secretlen, uint64_t n, const uint8_t* label,
                 size_t labellen, const uint8_t* seeds, size_t seedlen, size_t outlen, uint8_t* out, void* stream) {
    if (hashlen != 32 && hashlen != 48) return fail(TG_EINVAL, "hash length must be 32 or 48");
    if (int rc = tg::prf_args_error(secretlen, hashlen == 32 ? 64 : 128, labellen, label, seedlen, outlen, n)) return rc;
    if (n == 0) return TG_OK;
    if (!secrets || !out || (seedlen && !seeds)) return fail(TG_EINVAL, "null device buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const tg::PrfGeom g = tg::prf_geom(hashlen, labellen + seedlen);
    return tg::with_templates(
        tg::prf_pack_kernel, g, label, labellen, seeds, seedlen, nullptr, 0, n, s, "PRF template launch failed",
        "PRF launch failed", [&](const uint32_t* tmpl) {
            if (hashlen == 32)
                hipLaunchKernelGGL(tg::tls12_prf_kernel<tg::Sha256>, dim3(tg::blocks_of(n)), dim3(256), 0, s, tmpl,
                                   g.nb1, g.nb2, secrets, (uint32_t)secretlen, n, (uint32_t)outlen, out);
            else
                hipLaunchKernelGGL(tg::tls12_prf_kernel<tg::Sha384>, dim3(tg::blocks_of(n)), dim3(256), 0, s, tmpl,
                                   g.nb1, g.nb2, secrets, (uint32_t)secretlen, n, (uint32_t)outlen, out);
            return tg::launched() ? TG_OK : TG_EHIP;
        });
}

int tg_cbc_key_create_device(const uint8_t* enc_keys, size_t keylen, const uint8_t* mac_keys, size_t mackeylen,
                             int mac, size_t nkeys, tg_cbc_key** out, void* stream) {
    if (!out || !enc_keys || !mac_keys) return fail(TG_EINVAL, "null argument");
    char buf[80];
    if (const char* msg = tg::table_error(keylen, mackeylen, mac, nkeys, buf)) return fail(TG_EINVAL, "%s", msg);
    tg_cbc_key* k = new (std::nothrow) tg_cbc_key();
    if (!k) return fail(TG_ENOMEM, "out of host memory");
    k->rounds = keylen == 16 ? 10 : 14;
    k->mac = mac;
    k->nkeys = nkeys;
    k->dev_key = nullptr;
    k->stage = nullptr;
    k->stage_done = nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipGetDevice(&k->device);
    if (e == hipSuccess) e = hipMalloc((void**)&k->dev_key, nkeys * sizeof(tg::CbcKeyDev));
    int rc = e == hipSuccess ? TG_OK : fail(TG_EHIP, "cbc key alloc: %s", hipGetErrorString(e));
    if (!rc && tg::cbc_rows(k->rounds, mac, nullptr, enc_keys, mac_keys, mackeylen, nkeys, nkeys, k->dev_key, s))
        rc = fail(TG_EHIP, "cbc key setup launch failed");
    if (!rc && (e = hipStreamSynchronize(s)) != hipSuccess)
        rc = fail(TG_EHIP, "cbc key setup: %s", hipGetErrorString(e));
    if (rc) {
        if (k->dev_key) (void)hipFree(k->dev_key);
        delete k;
        return rc;
    }
    *out = k;
    return TG_OK;
}

int tg_cbc_key_replace_device(tg_cbc_key* k, const uint32_t* slot, const uint8_t* enc_keys, const uint8_t* mac_keys,
                              size_t mackeylen, uint64_t n, void* stream) {
    if (!k) return fail(TG_EINVAL, "null key");
    if (n > k->nkeys)
        return fail(TG_EINVAL, "%llu rows for a table of %zu keys", (unsigned long long)n, k->nkeys);
    if (n == 0) return TG_OK;
    if (!enc_keys || !mac_keys) return fail(TG_EINVAL, "null argument");
    char buf[80];
    if (const char* msg = tg::key_error(k->rounds == 10 ? 16 : 32, mackeylen, k->mac, buf))
        return fail(TG_EINVAL, "%s", msg);
    if (int rc = tg::cbc_select_device(k)) return rc;
    if (tg::cbc_rows(k->rounds, k->mac, slot, enc_keys, mac_keys, mackeylen, n, k->nkeys, k->dev_key,
                     static_cast<hipStream_t>(stream)))
        return fail(TG_EHIP, "cbc key replace launch failed");
    return TG_OK;
}

int tg_sessions_install_tls12(tg_key* k, const tg_tls12_install* r, void* stream) {
    if (int rc = tg::install_struct_error(r, true)) return rc;
    if (!k) return fail(TG_EINVAL, "null key");
    if (int rc = tg::install_count_error(r, k->nkeys)) return rc;
    if (!tg::aead_pair_ok(r->hashlen, k))
        return fail(TG_EINVAL, "no TLS 1.2 suite pairs the SHA-384 PRF with this handle (AES-256-GCM only)");
    if (r->n == 0) return TG_OK;
    if (int rc = tg::select_device(k)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const char* msg = "TLS 1.2 install launch failed";
    return tg::install_templates(r, s, msg, [&](const uint32_t* tmpl, const tg::PrfGeom& g) {
        return r->hashlen == 32 ? tg::launch_install<tg::Sha256>(k, tmpl, g, *r, s)
                                : tg::launch_install<tg::Sha384>(k, tmpl, g, *r, s);
    });
}

int tg_cbc_sessions_install_tls12(tg_cbc_key* k, const tg_tls12_install* r, void* stream) {
    if (int rc = tg::install_struct_error(r, false)) return rc;
    if (!k) return fail(TG_EINVAL, "null key");
    if (int rc = tg::install_count_error(r, k->nkeys)) return rc;
    if (!tg::cbc_pair_ok(r->hashlen, k))
        return fail(TG_EINVAL, "no TLS 1.2 suite pairs hashlen %u with this handle's key length and MAC", r->hashlen);
    if (r->n == 0) return TG_OK;
    if (int rc = tg::cbc_select_device(k)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const char* msg = "TLS 1.2 CBC install launch failed";
    return tg::install_templates(r, s, msg, [&](const uint32_t* tmpl, const tg::PrfGeom& g) {
        using namespace tg;
        if (r->hashlen == 48) return launch_cbc_install<Sha384, 8, Sha384>(k, tmpl, g, *r, s);
        if (k->mac == TG_MAC_SHA1)
            return k->rounds == 10 ? launch_cbc_install<Sha256, 4, Sha1>(k, tmpl, g, *r, s)
                                   : launch_cbc_install<Sha256, 8, Sha1>(k, tmpl, g, *r, s);
        return k->rounds == 10 ? launch_cbc_install<Sha256, 4, Sha256>(k, tmpl, g, *r, s)
                               : launch_cbc_install<Sha256, 8, Sha256>(k, tmpl, g, *r, s);
    });
}

}  // extern "C"
